// kernels_scan.hip -- brute-force distance scan kernels for gfx950.
//
// Two kernels replace faiss knn_L2sqr / knn_inner_product as called from
// VectorIndex::tryBruteForceSearch (BruteForceSearch.h:62-111):
//
//  * k_scan_small  (nq < 20, faiss exhaustive_*_seq): HBM-bound streaming scan.
//    A 256-thread workgroup owns 256 rows; row tiles of 32 floats are staged
//    through LDS with coalesced 16-B loads (double-buffered), then every lane
//    walks ITS row sequentially -- (x-y)^2 or x*y rounded then added, exactly
//    the fvec_* order the reference's KATs pin -- against up to 20 queries
//    whose values are wave-uniform (scalar loads).
//
//  * k_scan_mfma   (nq >= 20, faiss exhaustive_*_blas): MFMA-bound batch
//    contraction on v_mfma_f32_32x32x2_f32.  A 128x128 (rows x queries) tile
//    per workgroup, 4 waves of 64x64, K staged 32 deep through padded LDS.
//    The f32 MFMA is a k-ordered fma chain, i.e. the sgemm element the oracle
//    assumes; L2 uses (|x|^2 + |y|^2) - 2<x,y> clamped at 0.
//
// Neither kernel materialises the nq x n distance matrix.  A scan runs in
// one of two epilogue modes:
//    PROBE  -- write raw values for a short prefix of rows (the probe), from
//              which the k-th key per query gives an upper-bound threshold;
//    APPEND -- append only (raw, row) with key <= threshold to a per-query
//              candidate list (a few thousand entries).
// Validity (PREWHERE bitmap, lightweight-delete mask, empty arrays, metric
// quirks) is applied in the epilogue; see flat_kernels.h key32().
#include "flat_kernels.h"

namespace mqvs {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static __device__ inline float nan_f() { return __builtin_nanf(""); }

// Wave-aggregated append: every lane of the wave calls this for the same
// query j (VALU kernel); one atomic per wave instead of one per row.
// pos: scan position (probe column); row: the row (-1 = gather padding);
// inrange: pos inside the scanned range; have: inrange and a real row.
template <int METRIC, bool PROBE>
__device__ inline void emit_wave(const ScanParams &p, int j, int64_t pos, int64_t row, bool inrange,
                                 bool have, bool valid, float raw) {
    if (PROBE) {
        if (inrange)
            p.probe[(int64_t)j * p.probe_ld + (pos - p.row_begin)] = (have && valid) ? raw : __builtin_nanf("");
        return;
    }
    const uint32_t key = key32<METRIC>(raw);
    const bool take = have && valid && key != 0xFFFFFFFFu && key <= p.tau[j];
    cand_append_wave(p.cand, p.cand_count, p.cand_cap, j, take, raw, (uint32_t)row);
}

template <int METRIC, bool PROBE>
__device__ inline void emit(const ScanParams &p, int j, int64_t pos, int64_t row, bool valid, float raw) {
    if (PROBE) {
        p.probe[(int64_t)j * p.probe_ld + (pos - p.row_begin)] = valid ? raw : nan_f();
    } else if (valid) {
        const uint32_t key = key32<METRIC>(raw);
        if (key != 0xFFFFFFFFu && key <= p.tau[j])
            cand_append_one(p.cand, p.cand_count, p.cand_cap, j, raw, (uint32_t)row);
    }
}

// ---------------------------------------------------------------------------
// VALU scan, nq < 20.
constexpr int SB_K = 32;            // floats per stage
constexpr int SB_LD = SB_K + 4;     // padded LDS row (16-B aligned, conflict-free b128)

// One tile of the scan (the whole workgroup calls it with the same ti): the
// body k_scan_small and the part-group kernel k_scan_group share, so both
// compute a row's value with the same instructions.  tile / qtile: the
// workgroup's LDS stages, free on entry and on return.
template <int NQ, int METRIC, bool PROBE, bool VEC4>
__device__ __forceinline__ void scan_small_tile(const ScanParams &p, int64_t ti, float (*tile)[kSmallRows * SB_LD],
                                                float (*qtile)[NQ * SB_K]) {
    const int t = threadIdx.x;
    const int d = p.d;
    const int nst = (d + SB_K - 1) / SB_K;
    const int64_t qstride = (int64_t)((d + 31) / 32 * 32);
    // threads t < NQ*8 stage one float4 of the query slice per stage
    const int qj = t >> 3, qc = (t & 7) * 4;
    const bool qload = qj < NQ && qj < p.nq;
    {
        int64_t r0, r1, chunk;
        tile_range(p, ti, r0, r1, chunk);
        if (r0 >= r1) return;  // tile past the end of a partial last granule (block-uniform)
        const int ord = chunk_ordinal(p, chunk);
        const int64_t pos = r0 + t;
        const bool inrange = pos < r1;
        const int64_t row = inrange ? row_at(p, pos) : -1;
        const bool have = row >= 0;
        if (ord < 0) {  // chunk never searched by the reference (all arrays empty)
            if (PROBE && inrange)
                for (int j = 0; j < p.nq; ++j) emit<METRIC, true>(p, j, pos, row, false, 0.f);
            return;
        }
        const float *qsrc = qload
            ? p.qvars + ((int64_t)qj * p.maxv + variant_of(p, qj, ord)) * qstride + qc
            : nullptr;
        float acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] = 0.0f;

        float4 reg[8], qreg = make_float4(0.f, 0.f, 0.f, 0.f);
        auto load = [&](int s) {
            const int k0 = s * SB_K;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int f = t + 256 * i;
                const int lr = f >> 3, c = (f & 7) * 4;
                const int64_t gp = r0 + lr;
                const int64_t gr = gp < r1 ? row_at(p, gp) : -1;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gr >= 0) {
                    const float *src = p.rows + gr * d + k0 + c;
                    if (VEC4) {
                        if (k0 + c < d) v = *reinterpret_cast<const float4 *>(src);
                    } else {
                        if (k0 + c + 0 < d) v.x = src[0];
                        if (k0 + c + 1 < d) v.y = src[1];
                        if (k0 + c + 2 < d) v.z = src[2];
                        if (k0 + c + 3 < d) v.w = src[3];
                    }
                }
                reg[i] = v;
            }
            if (qload) qreg = *reinterpret_cast<const float4 *>(qsrc + k0);
        };
        auto store = [&](int b) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int f = t + 256 * i;
                const int lr = f >> 3, c = (f & 7) * 4;
                *reinterpret_cast<float4 *>(&tile[b][lr * SB_LD + c]) = reg[i];
            }
            if (t < NQ * 8) *reinterpret_cast<float4 *>(&qtile[b][qj * SB_K + qc]) = qreg;
        };
        load(0);
        store(0);
        __syncthreads();
        for (int s = 0; s < nst; ++s) {
            if (s + 1 < nst) load(s + 1);
            const float *tl = &tile[s & 1][t * SB_LD];
            const float *ql = qtile[s & 1];
#pragma unroll 2
            for (int kk = 0; kk < SB_K; kk += 4) {
                const float4 v = *reinterpret_cast<const float4 *>(tl + kk);
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    // same address in every lane: LDS broadcast
                    const float4 q = *reinterpret_cast<const float4 *>(ql + j * SB_K + kk);
                    if (METRIC == MQVS_METRIC_L2) {
                        float e;
                        e = v.x - q.x; acc[j] = acc[j] + e * e;
                        e = v.y - q.y; acc[j] = acc[j] + e * e;
                        e = v.z - q.z; acc[j] = acc[j] + e * e;
                        e = v.w - q.w; acc[j] = acc[j] + e * e;
                    } else {
                        acc[j] = acc[j] + v.x * q.x;
                        acc[j] = acc[j] + v.y * q.y;
                        acc[j] = acc[j] + v.z * q.z;
                        acc[j] = acc[j] + v.w * q.w;
                    }
                }
            }
            if (s + 1 < nst) store((s + 1) & 1);
            __syncthreads();
        }
        {
            const bool valid = have && row_valid(p, row);
#pragma unroll
            for (int j = 0; j < NQ; ++j)
                if (j < p.nq) emit_wave<METRIC, PROBE>(p, j, pos, row, inrange, have, valid, acc[j]);
        }
    }
}

template <int NQ, int METRIC, bool PROBE, bool VEC4>
__global__ __launch_bounds__(256) void k_scan_small(ScanParams p) {
    __shared__ __attribute__((aligned(16))) float tile[2][kSmallRows * SB_LD];
    __shared__ __attribute__((aligned(16))) float qtile[2][NQ * SB_K];
    for (int64_t ti = blockIdx.x; ti < p.tiles; ti += gridDim.x) scan_small_tile<NQ, METRIC, PROBE, VEC4>(p, ti, tile, qtile);
}

template <int NQ, int METRIC, bool PROBE>
static void launch_small_t(const ScanParams &p, hipStream_t s) {
    int64_t grid = p.tiles < 4096 ? p.tiles : 4096;
    if (grid < 1) return;
    if (p.d % 4 == 0)
        hipLaunchKernelGGL((k_scan_small<NQ, METRIC, PROBE, true>), dim3((unsigned)grid), dim3(256),
                           0, s, p);
    else
        hipLaunchKernelGGL((k_scan_small<NQ, METRIC, PROBE, false>), dim3((unsigned)grid), dim3(256),
                           0, s, p);
}

template <int METRIC, bool PROBE>
static void launch_small_m(const ScanParams &p, hipStream_t s) {
    const int nq = p.nq;
    if (nq <= 1) launch_small_t<1, METRIC, PROBE>(p, s);
    else if (nq <= 2) launch_small_t<2, METRIC, PROBE>(p, s);
    else if (nq <= 4) launch_small_t<4, METRIC, PROBE>(p, s);
    else if (nq <= 8) launch_small_t<8, METRIC, PROBE>(p, s);
    else if (nq <= 12) launch_small_t<12, METRIC, PROBE>(p, s);
    else if (nq <= 16) launch_small_t<16, METRIC, PROBE>(p, s);
    else launch_small_t<20, METRIC, PROBE>(p, s);
}

void launch_scan_small(const ScanParams &p, int metric, bool probe, hipStream_t s) {
    switch (metric) {
        case MQVS_METRIC_L2:
            probe ? launch_small_m<MQVS_METRIC_L2, true>(p, s) : launch_small_m<MQVS_METRIC_L2, false>(p, s);
            break;
        case MQVS_METRIC_IP:
            probe ? launch_small_m<MQVS_METRIC_IP, true>(p, s) : launch_small_m<MQVS_METRIC_IP, false>(p, s);
            break;
        case MQVS_METRIC_COSINE:
            probe ? launch_small_m<MQVS_METRIC_COSINE, true>(p, s)
                  : launch_small_m<MQVS_METRIC_COSINE, false>(p, s);
            break;
        default:
            probe ? launch_small_m<kMetricIpRaw, true>(p, s) : launch_small_m<kMetricIpRaw, false>(p, s);
            break;
    }
}

// ---------------------------------------------------------------------------
// Part-group scan (part_group.hip): k_scan_small's PROBE tiles over many small
// parts in one launch.  Tile ti of the launch belongs to the slot whose
// [tile0, next tile0) holds it (slots[nslots] is the sentinel); the workgroup
// takes that part's fields into its ScanParams and runs the shared tile body,
// so a row's value is the one mqvs_search computes for it.
template <int NQ, int METRIC, bool VEC4>
__global__ __launch_bounds__(256) void k_scan_group(ScanParams p, const GroupSlot *slots, int nslots, int64_t tiles) {
    __shared__ __attribute__((aligned(16))) float tile[2][kSmallRows * SB_LD];
    __shared__ __attribute__((aligned(16))) float qtile[2][NQ * SB_K];
    float *const matrix = p.probe;
    for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        // the last slot with tile0 <= ti (slots without tiles are skipped)
        int lo = 0, hi = nslots;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (slots[mid].tile0 <= ti) lo = mid;
            else hi = mid;
        }
        const GroupSlot &g = slots[lo];
        p.rows = g.rows;
        p.n = g.n;
        p.chunk_rows = g.granule;
        p.chunk_ord = g.chunk_ord;
        p.ord_base = (int)(g.row_offset / g.granule);
        p.filter = g.filter;
        p.exists = g.exists;
        p.nonempty = g.nonempty;
        p.row_begin = 0;
        p.row_end = g.n;
        p.tiles_per_chunk = g.tiles_per_chunk;
        p.tile_rows = kSmallRows;
        p.probe = matrix + g.col0;
        scan_small_tile<NQ, METRIC, true, VEC4>(p, ti - g.tile0, tile, qtile);
    }
}

template <int NQ, int METRIC>
static void launch_group_t(const ScanParams &p, const GroupSlot *slots, int nslots, int64_t tiles, hipStream_t s) {
    const int64_t grid = tiles < 4096 ? tiles : 4096;
    if (grid < 1) return;
    if (p.d % 4 == 0)
        hipLaunchKernelGGL((k_scan_group<NQ, METRIC, true>), dim3((unsigned)grid), dim3(256), 0, s, p, slots, nslots,
                           tiles);
    else
        hipLaunchKernelGGL((k_scan_group<NQ, METRIC, false>), dim3((unsigned)grid), dim3(256), 0, s, p, slots, nslots,
                           tiles);
}

template <int METRIC>
static void launch_group_m(const ScanParams &p, const GroupSlot *slots, int nslots, int64_t tiles, hipStream_t s) {
    const int nq = p.nq;
    if (nq <= 1) launch_group_t<1, METRIC>(p, slots, nslots, tiles, s);
    else if (nq <= 2) launch_group_t<2, METRIC>(p, slots, nslots, tiles, s);
    else if (nq <= 4) launch_group_t<4, METRIC>(p, slots, nslots, tiles, s);
    else if (nq <= 8) launch_group_t<8, METRIC>(p, slots, nslots, tiles, s);
    else if (nq <= 12) launch_group_t<12, METRIC>(p, slots, nslots, tiles, s);
    else if (nq <= 16) launch_group_t<16, METRIC>(p, slots, nslots, tiles, s);
    else launch_group_t<20, METRIC>(p, slots, nslots, tiles, s);
}

void launch_scan_group(const ScanParams &base, const GroupSlot *slots, int nslots, int64_t tiles, int metric,
                       hipStream_t s) {
    switch (metric) {
        case MQVS_METRIC_L2: launch_group_m<MQVS_METRIC_L2>(base, slots, nslots, tiles, s); break;
        case MQVS_METRIC_IP: launch_group_m<MQVS_METRIC_IP>(base, slots, nslots, tiles, s); break;
        default: launch_group_m<MQVS_METRIC_COSINE>(base, slots, nslots, tiles, s); break;
    }
}

// ---------------------------------------------------------------------------
// MFMA scan, nq >= 20.
constexpr int MB_K = 32;          // K per stage
constexpr int MB_LD = MB_K + 1;   // odd LDS row stride: conflict-free ds_read_b32 columns

// XCD-aware block -> logical work item l of L = tiles x query blocks (false:
// a block of the grid's round-up): the query blocks of one row tile are
// consecutive logical items and land on one XCD (same L2).
__device__ __forceinline__ bool mfma_block_item(int64_t tiles, int num_qblocks, int64_t &ti, int &qb) {
    const int64_t L = tiles * num_qblocks;
    const int64_t cpx = (L + 7) / 8;
    const int64_t b = blockIdx.x;
    const int64_t l = (b % 8) * cpx + b / 8;
    if (l >= L) return false;
    ti = l / num_qblocks;
    qb = (int)(l % num_qblocks);
    return true;
}

// One (row tile ti, query block qb) of the scan (the whole workgroup calls it
// with the same ti and qb): the body k_scan_mfma and the part-group kernel
// k_scan_group_mfma share, so both compute a row's value with the same
// instructions.  Ys / Qs: the workgroup's LDS stages, free on entry.
template <int METRIC, bool PROBE, bool VEC4>
__device__ __forceinline__ void scan_mfma_tile(const ScanParams &p, int64_t ti, int qb, float (*Ys)[kMfmaRows * MB_LD],
                                               float (*Qs)[kMfmaQ * MB_LD]) {
    int64_t r0, r1, chunk;
    tile_range(p, ti, r0, r1, chunk);
    if (r0 >= r1) return;  // tile past the end of a partial last granule
    const int ord = chunk_ordinal(p, chunk);
    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wr = w >> 1, wq = w & 1;
    const int h = lane >> 5, l32 = lane & 31;
    const int q0 = qb * kMfmaQ;
    const int d = p.d;
    const int64_t qstride = (int64_t)((d + 31) / 32 * 32);

    if (ord < 0) {
        if (PROBE) {
            for (int i = t; i < kMfmaRows * kMfmaQ; i += 256) {
                const int64_t row = r0 + (i % kMfmaRows);
                const int j = q0 + i / kMfmaRows;
                if (row < r1 && j < p.nq) emit<METRIC, true>(p, j, row, row, false, 0.f);
            }
        }
        return;
    }

    // per-thread global load slots: 4 float4 of Y and 4 of Q per stage
    const float *qsrc[4];
    bool qok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = t + 256 * i;
        const int lq = f >> 3;
        const int j = q0 + lq;
        qok[i] = j < p.nq;
        const int jj = qok[i] ? j : 0;
        qsrc[i] = p.qvars + ((int64_t)jj * p.maxv + variant_of(p, jj, ord)) * qstride + (f & 7) * 4;
    }
    float4 ry[4], rq[4];
    auto load = [&](int s) {
        const int k0 = s * MB_K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + 256 * i;
            const int lr = f >> 3, c = (f & 7) * 4;
            const int64_t gr = r0 + lr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr < r1) {
                const float *src = p.rows + gr * d + k0 + c;
                if (VEC4) {
                    if (k0 + c < d) v = *reinterpret_cast<const float4 *>(src);
                } else {
                    if (k0 + c + 0 < d) v.x = src[0];
                    if (k0 + c + 1 < d) v.y = src[1];
                    if (k0 + c + 2 < d) v.z = src[2];
                    if (k0 + c + 3 < d) v.w = src[3];
                }
            }
            ry[i] = v;
            rq[i] = qok[i] ? *reinterpret_cast<const float4 *>(qsrc[i] + k0)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int bf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + 256 * i;
            const int lr = f >> 3, c = (f & 7) * 4;
            float *ys = &Ys[bf][lr * MB_LD + c];
            ys[0] = ry[i].x; ys[1] = ry[i].y; ys[2] = ry[i].z; ys[3] = ry[i].w;
            float *qs = &Qs[bf][lr * MB_LD + c];
            qs[0] = rq[i].x; qs[1] = rq[i].y; qs[2] = rq[i].z; qs[3] = rq[i].w;
        }
    };

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    const int nst = (d + MB_K - 1) / MB_K;
    load(0);
    store(0);
    __syncthreads();
    const int ya = (wr * 64 + l32) * MB_LD + h;
    const int qa = (wq * 64 + l32) * MB_LD + h;
    for (int s = 0; s < nst; ++s) {
        if (s + 1 < nst) load(s + 1);
        const float *ys = Ys[s & 1];
        const float *qs = Qs[s & 1];
#pragma unroll
        for (int ks = 0; ks < MB_K / 2; ++ks) {
            const float a0 = ys[ya + 2 * ks];
            const float a1 = ys[ya + 32 * MB_LD + 2 * ks];
            const float b0 = qs[qa + 2 * ks];
            const float b1 = qs[qa + 32 * MB_LD + 2 * ks];
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
        if (s + 1 < nst) store((s + 1) & 1);
        __syncthreads();
    }

    // epilogue: lane holds query column l32 of each 32x32 block, 16 rows
    auto epi = [&](const f32x16 &acc, int rb, int qb2) {
        const int j = q0 + wq * 64 + qb2 * 32 + l32;
        if (j >= p.nq) return;
        const float qn = (METRIC == MQVS_METRIC_L2) ? p.qnorms[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int il = wr * 64 + rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t row = r0 + il;
            if (row >= r1) continue;
            float raw = acc[r];
            if (METRIC == MQVS_METRIC_L2) {
                raw = (qn + p.row_norms[row]) - 2.0f * acc[r];
                if (raw < 0) raw = 0;
            }
            emit<METRIC, PROBE>(p, j, row, row, row_valid(p, row), raw);
        }
    };
    epi(acc00, 0, 0);
    epi(acc01, 0, 1);
    epi(acc10, 1, 0);
    epi(acc11, 1, 1);
}

template <int METRIC, bool PROBE, bool VEC4>
__global__ __launch_bounds__(256, 2) void k_scan_mfma(ScanParams p) {
    __shared__ float Ys[2][kMfmaRows * MB_LD];
    __shared__ float Qs[2][kMfmaQ * MB_LD];
    int64_t ti;
    int qb;
    if (!mfma_block_item(p.tiles, p.num_qblocks, ti, qb)) return;
    scan_mfma_tile<METRIC, PROBE, VEC4>(p, ti, qb, Ys, Qs);
}

// Part-group batch scan (part_group.hip): k_scan_mfma's PROBE work items over
// many parts in one launch.  One (row tile, query block) per workgroup, so the
// body's returns and barriers stay block-uniform; tile ti of the launch
// belongs to the slot whose [tile0, next tile0) holds it, tiles counted in
// kMfmaRows rows (slots[nslots] is the sentinel).  The workgroup takes that
// part's fields into its ScanParams and runs the shared body, so a row's
// value is the one mqvs_search's fp32 batch scan computes for it.
template <int METRIC, bool VEC4>
__global__ __launch_bounds__(256, 2) void k_scan_group_mfma(ScanParams p, const GroupSlot *slots, int nslots,
                                                            int64_t tiles) {
    __shared__ float Ys[2][kMfmaRows * MB_LD];
    __shared__ float Qs[2][kMfmaQ * MB_LD];
    int64_t ti;
    int qb;
    if (!mfma_block_item(tiles, p.num_qblocks, ti, qb)) return;
    // the last slot with tile0 <= ti (slots without tiles are skipped)
    int lo = 0, hi = nslots;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (slots[mid].tile0 <= ti) lo = mid;
        else hi = mid;
    }
    const GroupSlot &g = slots[lo];
    p.rows = g.rows;
    p.row_norms = g.row_norms;
    p.n = g.n;
    p.chunk_rows = g.granule;
    p.chunk_ord = g.chunk_ord;
    p.ord_base = (int)(g.row_offset / g.granule);
    p.filter = g.filter;
    p.exists = g.exists;
    p.nonempty = g.nonempty;
    p.row_begin = 0;
    p.row_end = g.n;
    p.tiles_per_chunk = g.tiles_per_chunk;
    p.tile_rows = kMfmaRows;
    p.probe = p.probe + g.col0;
    scan_mfma_tile<METRIC, true, VEC4>(p, ti - g.tile0, qb, Ys, Qs);
}

template <int METRIC>
static void launch_group_mfma_t(const ScanParams &p, const GroupSlot *slots, int nslots, int64_t tiles,
                                hipStream_t s) {
    const int64_t L = tiles * p.num_qblocks;
    const int64_t grid = (L + 7) / 8 * 8;
    if (L < 1) return;
    if (grid > 0x7FFFFFFF) fail(MQVS_ERR_BAD_ARGUMENTS, "part group batch scan: more work items than one launch holds");
    if (p.d % 4 == 0)
        hipLaunchKernelGGL((k_scan_group_mfma<METRIC, true>), dim3((unsigned)grid), dim3(256), 0, s, p, slots, nslots,
                           tiles);
    else
        hipLaunchKernelGGL((k_scan_group_mfma<METRIC, false>), dim3((unsigned)grid), dim3(256), 0, s, p, slots,
                           nslots, tiles);
}

void launch_scan_group_mfma(const ScanParams &base, const GroupSlot *slots, int nslots, int64_t tiles, int metric,
                            hipStream_t s) {
    switch (metric) {
        case MQVS_METRIC_L2: launch_group_mfma_t<MQVS_METRIC_L2>(base, slots, nslots, tiles, s); break;
        case MQVS_METRIC_IP: launch_group_mfma_t<MQVS_METRIC_IP>(base, slots, nslots, tiles, s); break;
        default: launch_group_mfma_t<MQVS_METRIC_COSINE>(base, slots, nslots, tiles, s); break;
    }
}

template <int METRIC, bool PROBE>
static void launch_mfma_t(const ScanParams &p, hipStream_t s) {
    const int64_t L = p.tiles * p.num_qblocks;
    const int64_t grid = (L + 7) / 8 * 8;
    if (L < 1) return;
    if (p.d % 4 == 0)
        hipLaunchKernelGGL((k_scan_mfma<METRIC, PROBE, true>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((k_scan_mfma<METRIC, PROBE, false>), dim3((unsigned)grid), dim3(256), 0, s, p);
}

void launch_scan_mfma(const ScanParams &p, int metric, bool probe, hipStream_t s) {
    switch (metric) {
        case MQVS_METRIC_L2:
            probe ? launch_mfma_t<MQVS_METRIC_L2, true>(p, s) : launch_mfma_t<MQVS_METRIC_L2, false>(p, s);
            break;
        case MQVS_METRIC_IP:
            probe ? launch_mfma_t<MQVS_METRIC_IP, true>(p, s) : launch_mfma_t<MQVS_METRIC_IP, false>(p, s);
            break;
        case MQVS_METRIC_COSINE:
            probe ? launch_mfma_t<MQVS_METRIC_COSINE, true>(p, s)
                  : launch_mfma_t<MQVS_METRIC_COSINE, false>(p, s);
            break;
        default:
            probe ? launch_mfma_t<kMetricIpRaw, true>(p, s) : launch_mfma_t<kMetricIpRaw, false>(p, s);
            break;
    }
}

}  // namespace mqvs
