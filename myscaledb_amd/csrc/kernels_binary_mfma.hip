// kernels_binary_mfma.hip -- binary vectors on the matrix cores: the opt-in
// batch scan of the FLAT binary search (mqvs_set_binary_batch) and the opt-in
// assignment pass of the binary index build (assign=mfma).
//
// The bits of a code are 0/1 integers, so with both operands expanded to 0/1
// bytes v_mfma_i32_16x16x64_i8 accumulates dot = popcount(x & q) exactly, and
// every binary distance is an integer expression of dot, |x| and |q|:
//   Hamming  popcount(x ^ q) = |x| + |q| - 2 dot
//   Jaccard  num = dot, den = popcount(x | q) = |x| + |q| - dot
// Nothing is rounded, so the kernels here return the bits of the popcount
// kernels (kernels_binary.hip, k_bivf_assign) for every input.
//
// Operands.  Columns (queries, centroids) are expanded once per call by
// k_bin_expand into an i8 plane [columns padded to 16][K] (K = code_words * 32
// bytes: byte k of a column = bit k of its code) with |q| per column; a
// workgroup stages a tile of up to 128 columns x up to 512 bytes of it in LDS.  Rows stay
// packed in HBM: a lane reads one 32-bit word of its row per 128 code bits
// and spreads 16 bits to 16 bytes in registers (binary_spread.h) per MFMA.
// The dot product does not depend on the order of k as long as rows and
// columns agree: lane group g = lane >> 4 takes bits [32 g + 16 s, + 16) of a
// 128-bit piece in k-step s = 0, 1, on both sides.  |x| is a popcount of the
// packed words, kept in a per-wave LDS table for the epilogues.
//
// Tile.  256 threads, each wave 64 rows x 16 NB columns: 4 x NB blocks of
// 16 x 16 (NB = 8: 32 i32x4 accumulators; batches of up to 32 / 64 queries
// take NB = 2 / 4).  C/D map: column = lane & 15, rows
// 4 (lane >> 4) + reg -- a lane's column is its query / centroid, so the
// epilogues keep thresholds and |q| in per-lane registers, one per column
// block, and a lane's four values of a block are four consecutive rows.
// Workgroup w takes column tile w % nct and row tiles w / nct + i * stride:
// workgroups running together share rows (L2), and when K <= 512 the column
// tile is staged once per workgroup.  Longer codes stream the plane in
// 512-byte K chunks per row tile.
//
// Epilogues: PROBE (dense values), APPEND (k_scan_binary's tests, expression
// for expression; a block is walked only when one of its values passes the
// lane's threshold) and the index build's arg-min (k_bivf_assign's rule:
// smallest distance, lowest list id among equals).
#include "binary_spread.h"
#include "index_kernels.h"

namespace mqvs {

typedef int bm_i32x4 __attribute__((ext_vector_type(4)));

constexpr int kBmMB = 4;                       // 16-row blocks per wave
constexpr int kBmNB = 8;                       // 16-column blocks per column tile
constexpr int kBmWaveRows = 16 * kBmMB;        // 64
constexpr int kBmRows = 4 * kBmWaveRows;       // rows per workgroup tile
constexpr int kBmCols = 16 * kBmNB;            // columns per tile
constexpr int kBmKC = 512;                     // code bits (= plane bytes per column) per staged chunk
// LDS of a workgroup: the staged chunk of its 16 NB columns (NB 8: 64 KiB) and
// |x| of the tile's rows
constexpr int bm_plane_lds(int nb) { return 16 * nb * kBmKC; }
constexpr int bm_lds(int nb) { return bm_plane_lds(nb) + kBmRows * 4; }
static_assert(kBmKC % 128 == 0, "whole 128-bit pieces");
static_assert(kBmCols <= 128, "the arg-min key keeps the column in 7 bits");

// plane[col][k] = bit k of column col (0 / 1 bytes), zeros for the padding
// columns [ncols, ncols rounded up to 16); pop[col] = |q|
__global__ __launch_bounds__(256) void k_bin_expand(const uint32_t *codes, int ncols, int code_words, uint8_t *plane,
                                                    uint32_t *pop) {
    const int ncp = (ncols + 15) & ~15;
    const int64_t total = (int64_t)ncp * code_words;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t col = i / code_words;
        const int w = (int)(i % code_words);
        const uint32_t word = col < ncols ? codes[i] : 0u;
        uint32_t lo[4], hi[4];
        bin_spread16(word, lo);
        bin_spread16(word >> 16, hi);
        uint4 *dst = reinterpret_cast<uint4 *>(plane + i * 32);
        dst[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        dst[1] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        if (w == 0) {
            uint32_t c = 0;
            if (col < ncols)
                for (int u = 0; u < code_words; ++u) c += __builtin_popcount(codes[col * code_words + u]);
            pop[col] = c;
        }
    }
}

void launch_bin_expand(const uint32_t *codes, int ncols, int code_words, uint8_t *plane, uint32_t *pop,
                       hipStream_t s) {
    if (ncols <= 0) return;
    const int64_t total = (int64_t)((ncols + 15) & ~15) * code_words;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_bin_expand, dim3(grid), dim3(256), 0, s, codes, ncols, code_words, plane, pop);
}

// ---------------------------------------------------------------------------
// LDS image of a staged chunk: [128-bit piece u][column][128 B], the eight
// 16-B parts of a column's piece xor-swizzled by (column >> 1) & 7 so that the
// 16 lanes of a lane group (16 columns, one part) read 16 different bank
// groups.
template <int NB>
__device__ __forceinline__ int bm_lds_off(int u, int col, int part) {
    return ((u * (16 * NB) + col) << 7) + ((part ^ ((col >> 1) & 7)) << 4);
}

// columns [c0, c0 + 16 NB) x plane bytes [kb, kb + kcb) into the LDS image
// (columns past ncp: zeros).  The whole workgroup calls it between barriers.
template <int NB>
__device__ __forceinline__ void bm_stage(const uint8_t *plane, int ncp, int K, int c0, int kb, int kcb,
                                         unsigned char *lds) {
    const int ppc = kcb >> 4;  // 16-B parts per column
    const int total = 16 * NB * ppc;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int col = i / ppc, k16 = i % ppc;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c0 + col < ncp) v = *reinterpret_cast<const uint4 *>(plane + (int64_t)(c0 + col) * K + kb + (k16 << 4));
        *reinterpret_cast<uint4 *>(lds + bm_lds_off<NB>(k16 >> 3, col, k16 & 7)) = v;
    }
}

// |x| of the wave's 64 rows (row rw0 + lane; 0 past r1) into its LDS table
__device__ __forceinline__ void bm_row_pop(const uint32_t *codes, int code_words, int64_t rw0, int64_t r1,
                                           uint32_t *xs) {
    const int lane = threadIdx.x & 63;
    const int64_t row = rw0 + lane;
    uint32_t pc = 0;
    if (row < r1) {
        const uint4 *y = reinterpret_cast<const uint4 *>(codes + row * code_words);
        for (int u = 0; u < code_words / 4; ++u) {
            const uint4 v = y[u];
            pc += __builtin_popcount(v.x) + __builtin_popcount(v.y) + __builtin_popcount(v.z) + __builtin_popcount(v.w);
        }
    }
    xs[lane] = pc;
}

// acc[mb][nb] += (rows rw0 + 16 mb .. + 16) x (columns 16 nb .. + 16 of the
// staged tile) over code words [kw0, kw0 + 4 nu): i32 dot products.  Rows at
// or past r1 count as zero codes.
template <int NB>
__device__ __forceinline__ void bin_mfma_tile(const uint32_t *codes, int code_words, int64_t rw0, int64_t r1, int kw0,
                                              int nu, const unsigned char *lds, bm_i32x4 (&acc)[kBmMB][NB]) {
    constexpr int NU = kBmKC / 128;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    uint32_t aw[NU][kBmMB];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
        for (int mb = 0; mb < kBmMB; ++mb) {
            const int64_t row = rw0 + 16 * mb + c;
            aw[u][mb] = (u < nu && row < r1) ? codes[row * code_words + kw0 + 4 * u + g] : 0u;
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u >= nu) break;  // wave-uniform
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bm_i32x4 bf[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                bf[nb] = *reinterpret_cast<const bm_i32x4 *>(lds + bm_lds_off<NB>(u, 16 * nb + c, 2 * g + s));
#pragma unroll
            for (int mb = 0; mb < kBmMB; ++mb) {
                uint32_t sp[4];
                bin_spread16(aw[u][mb] >> (16 * s), sp);
                const bm_i32x4 af = {(int)sp[0], (int)sp[1], (int)sp[2], (int)sp[3]};
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[nb], acc[mb][nb], 0, 0, 0);
            }
        }
    }
}

// the dot products of one row tile against the workgroup's column tile, all K
// chunks; `staged`: the (single) chunk is already in LDS
template <int NB>
__device__ __forceinline__ void bm_tile_dots(const uint32_t *codes, int code_words, int64_t rw0, int64_t r1,
                                             const uint8_t *plane, int ncp, int c0, bool &staged,
                                             unsigned char *lds, bm_i32x4 (&acc)[kBmMB][NB]) {
    const int K = code_words * 32;
    const int nchunks = (K + kBmKC - 1) / kBmKC;
#pragma unroll
    for (int mb = 0; mb < kBmMB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = bm_i32x4{0, 0, 0, 0};
    for (int kc = 0; kc < nchunks; ++kc) {
        const int kb = kc * kBmKC;
        const int kcb = K - kb < kBmKC ? K - kb : kBmKC;
        if (nchunks > 1 || !staged) {  // (block-uniform)
            __syncthreads();
            bm_stage<NB>(plane, ncp, K, c0, kb, kcb, lds);
            __syncthreads();
            staged = true;
        }
        bin_mfma_tile<NB>(codes, code_words, rw0, r1, kb >> 5, kcb >> 7, lds, acc);
    }
}

// ---------------------------------------------------------------------------
// The batch scan of search_binary: k_scan_binary's PROBE values and APPEND
// candidates of rows [row_begin, row_end) for all nq queries.
template <int METRIC, bool PROBE, int NB>
__global__ __launch_bounds__(256, NB == kBmNB ? 1 : 2) void k_scan_binary_mfma(ScanParams p, BinPlane q, int64_t rtiles, int nct) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[bm_lds(NB)];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *xs = reinterpret_cast<uint32_t *>(lds + bm_plane_lds(NB)) + wave * kBmWaveRows;
    const int ct = blockIdx.x % nct;
    const int64_t rstride = gridDim.x / nct;
    const int c0 = ct * 16 * NB;
    const int ncp = (p.nq + 15) & ~15;
    const int nbits = p.nbits;

    // the lane's column of each block: |q| and, APPEND, its thresholds.  The
    // per-lane flags (column is a query: jokm; its tau takes all: allm) are
    // bits of an integer: as bools each would hold a lane mask in a scalar
    // register pair for the whole kernel.
    uint32_t qs[NB], tauv[NB];
    int lim[NB];
    float tfv[NB];
    uint32_t jokm = 0u, allm = 0u;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int j = c0 + 16 * nb + c;
        jokm |= (j < p.nq ? 1u : 0u) << nb;
        qs[nb] = j < ncp ? q.pop[j] : 0u;
        tauv[nb] = 0u;
        lim[nb] = 0;
        tfv[nb] = 0.f;
        if (!PROBE && j < p.nq) {
            // as k_scan_binary: keys of the non-negative values are ord_asc =
            // bits | 2^31, and a tau of 0xFFFFFFFE / 0xFFFFFFFF takes all
            const uint32_t tau = p.tau[j];
            const bool all = tau >= 0xFFFFFFFEu;
            const float tf = __builtin_bit_cast(float, tau & 0x7FFFFFFFu);
            tauv[nb] = tau;
            allm |= (all ? 1u : 0u) << nb;
            tfv[nb] = tf;
            // integer limit: h < ceil(tf) (strict) or h <= floor(tf)
            int l = nbits;
            if (!all && tf < (float)nbits) l = p.tau_strict ? (int)ceilf(tf) : (int)floorf(tf) + 1;
            lim[nb] = l;
        }
    }
    const bool vec_ok = (p.probe_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(p.probe) & 15) == 0;

    bool staged = false;
    for (int64_t rt = blockIdx.x / nct; rt < rtiles; rt += rstride) {
        const int64_t r0 = p.row_begin + rt * kBmRows;
        const int64_t r1 = r0 + kBmRows < p.row_end ? r0 + kBmRows : p.row_end;
        const int64_t rw0 = r0 + (int64_t)wave * kBmWaveRows;
        bm_row_pop(p.codes, p.code_words, rw0, r1, xs);
        bm_i32x4 acc[kBmMB][NB];
        bm_tile_dots<NB>(p.codes, p.code_words, rw0, r1, q.plane, ncp, c0, staged, lds, acc);

#pragma unroll
        for (int mb = 0; mb < kBmMB; ++mb) {
            const int64_t pos0 = rw0 + 16 * mb + 4 * g;
            const uint4 xv = *reinterpret_cast<const uint4 *>(xs + 16 * mb + 4 * g);
            const uint32_t x4[4] = {xv.x, xv.y, xv.z, xv.w};
            // (the flag words pass through an empty asm: otherwise the tests of
            // their bits are hoisted out of the row-tile loop as one lane mask
            // per bit, and the scalar registers run out)
            asm volatile("" : "+v"(jokm), "+v"(allm));
            if (PROBE) {
                uint32_t vrm = 0u;
#pragma unroll
                for (int r = 0; r < 4; ++r) vrm |= (pos0 + r < r1 && row_valid(p, pos0 + r) ? 1u : 0u) << r;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    if (!((jokm >> nb) & 1u)) continue;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t dot = (uint32_t)acc[mb][nb][r];
                        const uint32_t a = METRIC == MQVS_METRIC_HAMMING ? x4[r] + qs[nb] - 2u * dot : dot;
                        const uint32_t b = METRIC == MQVS_METRIC_HAMMING ? 0u : x4[r] + qs[nb] - dot;
                        v[r] = bin_probe_value<METRIC>(a, b, (vrm >> r) & 1u, nbits);
                    }
                    float *dst = p.probe + (int64_t)(c0 + 16 * nb + c) * p.probe_ld + (pos0 - p.row_begin);
                    if (vec_ok && pos0 + 3 < r1) {
                        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (pos0 + r < r1) dst[r] = v[r];
                    }
                }
            } else {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    uint32_t a[4], b[4];
                    uint32_t hm = 0u;  // bit r: row r of the block passes the lane's threshold
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t dot = (uint32_t)acc[mb][nb][r];
                        if (METRIC == MQVS_METRIC_HAMMING) {
                            a[r] = x4[r] + qs[nb] - 2u * dot;
                            b[r] = 0u;
                            hm |= ((int)a[r] < lim[nb] ? 1u : 0u) << r;  // (lim 0: not a query)
                        } else {
                            // cheap superset test first, exact fp32 division for the few that pass
                            a[r] = dot;
                            b[r] = x4[r] + qs[nb] - dot;
                            const float dn = (float)(b[r] - a[r]), dd = (float)b[r];
                            hm |= (((allm >> nb) & 1u) || a[r] == 0u || dn <= tfv[nb] * dd * 1.0000005f ? 1u : 0u) << r;
                        }
                    }
                    if (hm == 0u || !((jokm >> nb) & 1u)) continue;
                    // the rare path, kept small (one copy per block, a loop
                    // over its rows: the selects keep a / b in registers)
                    const int j = c0 + 16 * nb + c;
#pragma unroll 1
                    for (int r = 0; r < 4; ++r) {
                        const bool h = (hm >> r) & 1u;
                        const uint32_t ar = r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3];
                        const uint32_t br = r == 0 ? b[0] : r == 1 ? b[1] : r == 2 ? b[2] : b[3];
                        const int64_t pos = pos0 + r;
                        bool take = h && pos < r1 && row_valid(p, pos);
                        float raw;
                        if (METRIC == MQVS_METRIC_HAMMING) {
                            raw = (float)ar;
                        } else {
                            const float dn = (float)(br - ar), dd = (float)br;
                            raw = ar == 0u ? 1.0f : dn / dd;
                            const uint32_t key = ord_asc(raw);
                            take = take && (p.tau_strict ? key < tauv[nb] : key <= tauv[nb]);
                        }
                        // hits are rare after the probe: a slot per hit
                        // (the order inside a list is unspecified)
                        if (take) cand_append_one(p.cand, p.cand_count, p.cand_cap, j, raw, (uint32_t)pos);
                    }
                }
            }
        }
    }
}

template <int METRIC, bool PROBE, int NB>
static void scan_binary_mfma_nb(const ScanParams &p, const BinPlane &q, hipStream_t s) {
    const int64_t rtiles = (p.row_end - p.row_begin + kBmRows - 1) / kBmRows;
    if (rtiles <= 0 || p.nq <= 0) return;
    const int nct = (p.nq + 16 * NB - 1) / (16 * NB);
    // two workgroups fit a CU; a workgroup that keeps its column tile staged
    // should see several row tiles
    const int64_t rg = std::min<int64_t>(rtiles, std::max<int64_t>(1, 1024 / nct));
    hipLaunchKernelGGL((k_scan_binary_mfma<METRIC, PROBE, NB>), dim3((unsigned)(rg * nct)), dim3(256), 0, s, p,
                       q, rtiles, nct);
}

// column blocks per tile: the narrowest of 2 / 4 / 8 that holds the batch in
// one tile (a spread feeds NB MFMAs; padding columns cost whole MFMAs)
template <int METRIC, bool PROBE>
static void scan_binary_mfma_t(const ScanParams &p, const BinPlane &q, hipStream_t s) {
    if (p.nq <= 32)
        scan_binary_mfma_nb<METRIC, PROBE, 2>(p, q, s);
    else if (p.nq <= 64)
        scan_binary_mfma_nb<METRIC, PROBE, 4>(p, q, s);
    else
        scan_binary_mfma_nb<METRIC, PROBE, kBmNB>(p, q, s);
}

void launch_scan_binary_mfma(const ScanParams &p, const BinPlane &q, int metric, bool probe, hipStream_t s) {
    if (metric == MQVS_METRIC_HAMMING)
        probe ? scan_binary_mfma_t<MQVS_METRIC_HAMMING, true>(p, q, s)
              : scan_binary_mfma_t<MQVS_METRIC_HAMMING, false>(p, q, s);
    else
        probe ? scan_binary_mfma_t<MQVS_METRIC_JACCARD, true>(p, q, s)
              : scan_binary_mfma_t<MQVS_METRIC_JACCARD, false>(p, q, s);
}

// ---------------------------------------------------------------------------
// The index build's assignment: assign[r] = the centroid at the smallest
// Hamming distance of row r, the lowest list id among equals (a centroid at
// distance == nbits is a legitimate nearest list) -- k_bivf_assign's rule.
// A workgroup keeps a row tile and visits the column tiles in ascending list
// order: inside a tile the 16 column lanes reduce one integer key
// (distance << 7 | column of the tile), across tiles a strict < on the
// distance keeps the lower list.
__global__ __launch_bounds__(256, 1) void k_bivf_assign_mfma(const uint32_t *codes, int64_t n, int code_words,
                                                          const uint8_t *cplane, const uint32_t *cpop, int nlist,
                                                          int32_t *assign) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[bm_lds(kBmNB)];
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *xs = reinterpret_cast<uint32_t *>(lds + bm_plane_lds(kBmNB)) + wave * kBmWaveRows;
    const int ncp = (nlist + 15) & ~15;
    const int nct = (nlist + kBmCols - 1) / kBmCols;
    const int64_t rtiles = (n + kBmRows - 1) / kBmRows;
    for (int64_t rt = blockIdx.x; rt < rtiles; rt += gridDim.x) {
        const int64_t r0 = rt * kBmRows;
        const int64_t r1 = r0 + kBmRows < n ? r0 + kBmRows : n;
        const int64_t rw0 = r0 + (int64_t)wave * kBmWaveRows;
        bm_row_pop(codes, code_words, rw0, r1, xs);
        uint32_t best[kBmMB][4];
        int32_t arg[kBmMB][4];
#pragma unroll
        for (int mb = 0; mb < kBmMB; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                best[mb][r] = 0xFFFFFFFFu;
                arg[mb][r] = 0;
            }
        for (int ct = 0; ct < nct; ++ct) {
            const int c0 = ct * kBmCols;
            uint32_t qs[kBmNB];
            bool jok[kBmNB];
#pragma unroll
            for (int nb = 0; nb < kBmNB; ++nb) {
                const int j = c0 + 16 * nb + c;
                jok[nb] = j < nlist;
                qs[nb] = j < ncp ? cpop[j] : 0u;
            }
            bm_i32x4 acc[kBmMB][kBmNB];
            bool staged = false;  // every column tile is staged again
            bm_tile_dots<kBmNB>(codes, code_words, rw0, r1, cplane, ncp, c0, staged, lds, acc);
#pragma unroll
            for (int mb = 0; mb < kBmMB; ++mb) {
                const uint4 xv = *reinterpret_cast<const uint4 *>(xs + 16 * mb + 4 * g);
                const uint32_t x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    uint32_t key = 0xFFFFFFFFu;
#pragma unroll
                    for (int nb = 0; nb < kBmNB; ++nb) {
                        const uint32_t h = x4[r] + qs[nb] - 2u * (uint32_t)acc[mb][nb][r];
                        const uint32_t kk = jok[nb] ? (h << 7) | (uint32_t)(16 * nb + c) : 0xFFFFFFFFu;
                        key = kk < key ? kk : key;
                    }
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) {
                        const uint32_t other = (uint32_t)__shfl_xor((int)key, o);
                        key = other < key ? other : key;
                    }
                    if (key != 0xFFFFFFFFu && (key >> 7) < best[mb][r]) {
                        best[mb][r] = key >> 7;
                        arg[mb][r] = c0 + (int)(key & 127u);
                    }
                }
            }
        }
        if (c == 0) {
#pragma unroll
            for (int mb = 0; mb < kBmMB; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = rw0 + 16 * mb + 4 * g + r;
                    if (row < r1) assign[row] = arg[mb][r];
                }
        }
    }
}

// cplane / cpop: scratch for the expanded centroids, bin_plane_bytes(nlist,
// code_words) and nlist rounded up to 16 words
void launch_bivf_assign_mfma(const uint32_t *codes, int64_t n, int code_words, const uint32_t *cent, int nlist,
                             uint8_t *cplane, uint32_t *cpop, int32_t *assign, hipStream_t s) {
    if (n <= 0 || nlist <= 0) return;
    launch_bin_expand(cent, nlist, code_words, cplane, cpop, s);
    const int64_t rtiles = (n + kBmRows - 1) / kBmRows;
    const int grid = (int)std::min<int64_t>(rtiles, 1 << 16);
    hipLaunchKernelGGL(k_bivf_assign_mfma, dim3(grid), dim3(256), 0, s, codes, n, code_words, cplane, cpop, nlist,
                       assign);
}

}  // namespace mqvs
