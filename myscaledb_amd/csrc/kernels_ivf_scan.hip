// kernels_ivf_scan.hip -- the index search's two list scans (index_kernels.h
// has the overview): k_ivf_scan over a bf16 list plane, k_ivf_scan_fp8 over an
// fp8 one.
#include "index_kernels.h"

namespace mqvs {

typedef __bf16 ivf_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ivf_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIvfWin = 4;      // 64-column windows loaded per group in the scan

// Scan work item = one list x up to 16 QB queries (QB MFMA B blocks).  The
// query tile sits in LDS (row stride 2 dpad + 16 B: the 16 rows of a B block
// hit distinct bank groups).  Each wave takes 16-row blocks of the list; lane
// (l16, c) streams row l16 straight from HBM into A fragments: per 64-column
// window, k-step 1 = bytes [16c, 16c + 16), k-step 2 = [64 + 16c, ...), so
// one load instruction covers a contiguous 64-B half-window of 16 rows.
// kIvfWin windows are in flight per lane and the next group is prefetched
// while the current one feeds the MFMAs; every A fragment serves QB MFMAs.
template <int METRIC, int QB>
__global__ __launch_bounds__(256) void k_ivf_scan(IvfParams p) {
    constexpr int QG = 16 * QB;
    // plane reads: each probed list's rows are read once per query group
    // (non-temporal: kept out of the caches' retention)
    auto ldp = [](const uint16_t *a) __attribute__((always_inline)) {
        typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
        return __builtin_bit_cast(ivf_bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(a)));
    };
    extern __shared__ __attribute__((aligned(16))) unsigned char qtile[];  // QG x (2 dpad + 16) B
    __shared__ int s_ent[QG];
    __shared__ int64_t s_base[QG];
    __shared__ float s_qn[QG];
    const int64_t qstr = 2 * p.dpad + 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l16 = lane & 15, c = lane >> 4;
    const int nitems = p.pair_stride ? p.nq * p.nprobe * p.pair_nch : *p.nitems;
    const int cpr = (int)(p.dpad / 8);  // 16-B chunks per query row
    const int ngrp = (int)((p.dpad / 64 + kIvfWin - 1) / kIvfWin);
    for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
        int l, g, chk, pe = -1;
        if (p.pair_stride) {
            // pair mode: one query's probe; slices past its list's end are
            // empty.  Slice-major (slice 0 of every pair first): pair-major
            // gave the workgroups of the first slices two items each and the
            // rest none (scan 82 -> 169 us at nq 1000, nprobe 1)
            const int E = p.nq * p.nprobe;
            chk = it / E;
            pe = it - chk * E;
            g = 0;
            const int64_t ll = p.probes[pe];
            if (ll < 0 || ll >= p.nlist) continue;  // (uniform over the workgroup)
            l = (int)ll;
            if ((int64_t)chk * p.chunk >= p.list_off[l + 1] - p.list_off[l]) continue;
        } else {
            l = p.item_list[it];
            g = p.item_grp[it];
            chk = p.item_chk[it];
        }
        const int64_t pos0 = p.list_off[l];
        const int cb = p.chunk / 16;  // 16-position blocks per work item
        const int nb = (int)min<int64_t>((p.list_off[l + 1] - pos0) / 16, (int64_t)(chk + 1) * cb);
        // the wave's blocks b0, b0 + 4, ... as one sequence of (block, window
        // group) steps: the next step's loads -- the next block's first group
        // included -- are in flight while a step feeds the MFMAs
        const int b0 = chk * cb + w;
        const int nsteps = b0 < nb ? (nb - b0 + 3) / 4 * ngrp : 0;
        // the plane is blocked like the FLAT pre-filter plane: 16 positions x
        // 32 columns = 1 KiB per piece (k_ivf_pack), so each fragment load of a
        // wave reads one contiguous KiB (8 whole 128-B lines)
        const uint16_t *rp0 = p.plane + ((pos0 >> 4) + (int64_t)b0) * 16 * p.dpad + l16 * 32 + c * 8;
        const int64_t bstride = 4 * 16 * p.dpad;  // 4 blocks on
        auto load = [&](int st, ivf_bf16x8 *dst) {
            const int bi = st / ngrp, grp = st - bi * ngrp;
            const uint16_t *rp = rp0 + bi * bstride;
#pragma unroll
            for (int u = 0; u < kIvfWin; ++u) {
                const int64_t kw = ((int64_t)grp * kIvfWin + u) * 64;
                if (kw < p.dpad) {
                    dst[2 * u] = ldp(rp + (kw >> 5) * 512);
                    dst[2 * u + 1] = ldp(rp + ((kw >> 5) + 1) * 512);
                }
            }
        };
        // the first step's rows are requested before the query tile is staged
        // (its chain of dependent loads: pairs, regions, query rows): at ~256
        // positions per list the item setup is a large part of an item
        ivf_bf16x8 cur[2 * kIvfWin], nxt[2 * kIvfWin];
        if (nsteps > 0) load(0, cur);
        const int cnt = p.pair_stride ? 1 : min(QG, p.lcount[l] - g * QG);
        __syncthreads();  // the previous item's readers are done with qtile
        if (threadIdx.x < QG) {
            const int j = threadIdx.x;
            int e = -1;
            int64_t base = 0;
            if (p.pair_stride) {
                // the pair's region: its query's stride, after the lists of
                // the query's earlier probes
                if (j == 0) {
                    e = pe;
                    const int q = e / p.nprobe, r = e - q * p.nprobe;
                    base = (int64_t)q * p.pair_stride;
                    for (int r2 = 0; r2 < r; ++r2) {
                        const int64_t l2 = p.probes[(int64_t)q * p.nprobe + r2];
                        if (l2 >= 0 && l2 < p.nlist) base += p.list_off[l2 + 1] - p.list_off[l2];
                    }
                }
            } else {
                e = j < cnt ? p.lq[p.lstart[l] + (int64_t)g * QG + j] : -1;
                base = e >= 0 ? p.qstart[e / p.nprobe] + p.qbase[e] : 0;
            }
            s_ent[j] = e;
            s_base[j] = base;
            s_qn[j] = (e >= 0 && METRIC == MQVS_METRIC_L2) ? p.qnorm[e / p.nprobe] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < QG * cpr; i += 256) {
            const int j = i / cpr, cc = i - j * cpr;
            const int e = s_ent[j];
            uint4 v = make_uint4(0, 0, 0, 0);
            if (e >= 0) v = reinterpret_cast<const uint4 *>(p.q_hi + (int64_t)(e / p.nprobe) * p.dpad)[cc];
            *reinterpret_cast<uint4 *>(qtile + j * qstr + cc * 16) = v;
        }
        __syncthreads();
        const unsigned char *qp = qtile + l16 * qstr + c * 16;
        int ent[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) ent[j] = s_ent[16 * j + l16];
        ivf_f32x4 acc[QB];
        int32_t rows[4];
        float pn[4];
        for (int st = 0; st < nsteps; ++st) {
            const int bi = st / ngrp, grp = st - bi * ngrp;
            const int64_t lp = (int64_t)(b0 + 4 * bi) * 16 + 4 * c;
            if (grp == 0) {
#pragma unroll
                for (int j = 0; j < QB; ++j) acc[j] = ivf_f32x4{0.f, 0.f, 0.f, 0.f};
                // the block's position records, ahead of the next step's loads
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    rows[r] = p.perm[pos0 + lp + r];
                    pn[r] = METRIC == MQVS_METRIC_L2 ? p.pnorm[pos0 + lp + r] : 0.f;
                }
            }
            if (st + 1 < nsteps) load(st + 1, nxt);
#pragma unroll
            for (int u = 0; u < kIvfWin; ++u) {
                const int64_t kw = ((int64_t)grp * kIvfWin + u) * 64;
                if (kw < p.dpad) {
#pragma unroll
                    for (int j = 0; j < QB; ++j) {
                        const unsigned char *qj = qp + 16 * j * qstr + 2 * kw;
                        const ivf_bf16x8 q0 = *reinterpret_cast<const ivf_bf16x8 *>(qj);
                        const ivf_bf16x8 q1 = *reinterpret_cast<const ivf_bf16x8 *>(qj + 64);
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur[2 * u], q0, acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur[2 * u + 1], q1, acc[j], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2 * kIvfWin; ++u) cur[u] = nxt[u];
            if (grp != ngrp - 1) continue;
            // C: lane (l16, c) holds rows 4c..4c+3 of the block for query slot 16 j + l16
            int32_t rr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int32_t row = rows[r];
                if (row >= 0 && p.filter && !bit_test(p.filter, row)) row = -1;
                if (row >= 0 && p.exists && !bit_test(p.exists, row)) row = -1;
                rr[r] = row;
            }
#pragma unroll
            for (int j = 0; j < QB; ++j) {
                if (ent[j] < 0) continue;
                Cand out[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float raw = acc[j][r];
                    if (METRIC == MQVS_METRIC_L2) raw = (s_qn[16 * j + l16] + pn[r]) - 2.0f * raw;
                    out[r].raw = rr[r] >= 0 ? raw : __builtin_nanf("");
                    out[r].row = rr[r] >= 0 ? (uint32_t)rr[r] : 0xFFFFFFFFu;
                }
                uint4 *dst = reinterpret_cast<uint4 *>(p.cand + s_base[16 * j + l16] + lp);
                dst[0] = *reinterpret_cast<const uint4 *>(&out[0]);
                dst[1] = *reinterpret_cast<const uint4 *>(&out[2]);
            }
        }
    }
}

// The same scan over an fp8 list plane (mqvs_index_build, plane=fp8): OCP
// e4m3fn codes with one scale exponent per position and per query.  Work
// items, prefetch sequence, non-temporal plane loads and the epilogue are
// k_ivf_scan's; only the bytes streamed halve.  The plane is blocked [npos /
// 16][dpad / 64][16][64] bytes, so a fragment load of a wave still reads one
// contiguous KiB: lane (l16, c) takes bytes [16c, 16c + 16) of row l16 of a
// 64-column window and feeds them as two k-steps (columns 16c .. 16c + 7 and
// 16c + 8 .. 16c + 15); the query tile in LDS is read in the same order (32
// contiguous bytes per lane and window), so both operands of a k-step hold
// the same columns.  kIvfWin8 windows per group: the bytes in flight per lane
// of the bf16 scan's group.
//
// The products are summed by the bf16 MFMA, not by v_mfma_f32_16x16x32_fp8_fp8:
// every e4m3 value is a bf16 value, so the codes are widened in registers
// (v_cvt_scalef32_pk_bf16_fp8 with scale 1: 8 VALU instructions per lane and
// window beside 2 QB MFMAs, in a kernel bound by HBM) and the query tile holds
// the queries' scaled codes as bf16.  The fp8 MFMA sums its 32 products in a
// window of about 13 bits under the largest one (measured on an MI355X,
// tools/fp8_mfma_probe.hip: up to 2^-10.7 of the largest product per
// instruction on random codes; 2^16 + 2^-7 gives 2^16) -- the accumulation
// term of k_query_bound, and a first stage pinned to 2.04 d u sum |p|, need
// the fp32 sum the bf16 MFMA gives.  The accumulator then holds the sum of
// the code products (each exact in fp32); the approximate inner product is
// that sum times 2^-(e_p + e_q), scaled in one step (v_ldexp_f32: the product
// of the two scales can leave the fp32 range where the result does not).  A
// result that is not finite is reported as NaN, which the select ranks first
// before a re-rank (the exact value decides) and leaves out of a first-stage
// result.
constexpr int kIvfWin8 = 8;
typedef uint32_t ivf_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ivf_bf16x2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn codes (two dwords) as the 8 bf16 values of an MFMA fragment
__device__ __forceinline__ ivf_bf16x8 ivf_widen8(uint32_t lo, uint32_t hi) {
    ivf_u32x4 w;
    w[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    w[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    w[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    w[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    return __builtin_bit_cast(ivf_bf16x8, w);
}

template <int METRIC, int QB>
__global__ __launch_bounds__(256) void k_ivf_scan_fp8(IvfParams p) {
    constexpr int QG = 16 * QB;
    auto ldp = [](const uint8_t *a) __attribute__((always_inline)) {
        return __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(a));
    };
    extern __shared__ __attribute__((aligned(16))) unsigned char qtile[];  // QG x (2 dpad + 16) B
    __shared__ int s_ent[QG];
    __shared__ int64_t s_base[QG];
    __shared__ float s_qn[QG];
    const int64_t qstr = 2 * p.dpad + 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l16 = lane & 15, c = lane >> 4;
    const int nitems = p.pair_stride ? p.nq * p.nprobe * p.pair_nch : *p.nitems;
    const int cpr = (int)(p.dpad / 8);  // 16-B chunks per query row
    const int ngrp = (int)((p.dpad / 64 + kIvfWin8 - 1) / kIvfWin8);
    for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
        int l, g, chk, pe = -1;
        if (p.pair_stride) {
            // pair mode, slice-major (see k_ivf_scan)
            const int E = p.nq * p.nprobe;
            chk = it / E;
            pe = it - chk * E;
            g = 0;
            const int64_t ll = p.probes[pe];
            if (ll < 0 || ll >= p.nlist) continue;  // (uniform over the workgroup)
            l = (int)ll;
            if ((int64_t)chk * p.chunk >= p.list_off[l + 1] - p.list_off[l]) continue;
        } else {
            l = p.item_list[it];
            g = p.item_grp[it];
            chk = p.item_chk[it];
        }
        const int64_t pos0 = p.list_off[l];
        const int cb = p.chunk / 16;  // 16-position blocks per work item
        const int nb = (int)min<int64_t>((p.list_off[l + 1] - pos0) / 16, (int64_t)(chk + 1) * cb);
        const int b0 = chk * cb + w;
        const int nsteps = b0 < nb ? (nb - b0 + 3) / 4 * ngrp : 0;
        // a block's 64-column window is one KiB piece: row l16 at 64 l16
        const uint8_t *rp0 = p.plane8 + ((pos0 >> 4) + (int64_t)b0) * 16 * p.dpad + l16 * 64 + c * 16;
        const int64_t bstride = 4 * 16 * p.dpad;  // 4 blocks on
        auto load = [&](int st, ivf_u32x4 *dst) {
            const int bi = st / ngrp, grp = st - bi * ngrp;
            const uint8_t *rp = rp0 + bi * bstride;
#pragma unroll
            for (int u = 0; u < kIvfWin8; ++u) {
                const int64_t kw = ((int64_t)grp * kIvfWin8 + u) * 64;
                if (kw < p.dpad) dst[u] = ldp(rp + (kw >> 6) * 1024);
            }
        };
        // the first step's rows are requested before the query tile is staged
        ivf_u32x4 cur[kIvfWin8], nxt[kIvfWin8];
        if (nsteps > 0) load(0, cur);
        const int cnt = p.pair_stride ? 1 : min(QG, p.lcount[l] - g * QG);
        __syncthreads();  // the previous item's readers are done with qtile
        if (threadIdx.x < QG) {
            const int j = threadIdx.x;
            int e = -1;
            int64_t base = 0;
            if (p.pair_stride) {
                if (j == 0) {
                    e = pe;
                    const int q = e / p.nprobe, r = e - q * p.nprobe;
                    base = (int64_t)q * p.pair_stride;
                    for (int r2 = 0; r2 < r; ++r2) {
                        const int64_t l2 = p.probes[(int64_t)q * p.nprobe + r2];
                        if (l2 >= 0 && l2 < p.nlist) base += p.list_off[l2 + 1] - p.list_off[l2];
                    }
                }
            } else {
                e = j < cnt ? p.lq[p.lstart[l] + (int64_t)g * QG + j] : -1;
                base = e >= 0 ? p.qstart[e / p.nprobe] + p.qbase[e] : 0;
            }
            s_ent[j] = e;
            s_base[j] = base;
            s_qn[j] = (e >= 0 && METRIC == MQVS_METRIC_L2) ? p.qnorm[e / p.nprobe] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < QG * cpr; i += 256) {
            const int j = i / cpr, cc = i - j * cpr;
            const int e = s_ent[j];
            uint4 v = make_uint4(0, 0, 0, 0);
            if (e >= 0) v = reinterpret_cast<const uint4 *>(p.q_hi + (int64_t)(e / p.nprobe) * p.dpad)[cc];
            *reinterpret_cast<uint4 *>(qtile + j * qstr + cc * 16) = v;
        }
        __syncthreads();
        const unsigned char *qp = qtile + l16 * qstr + c * 32;
        int ent[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) ent[j] = s_ent[16 * j + l16];
        int qe[QB];  // the slots' query scale exponents
#pragma unroll
        for (int j = 0; j < QB; ++j) qe[j] = ent[j] >= 0 ? (int)p.qexp[ent[j] / p.nprobe] : 0;
        ivf_f32x4 acc[QB];
        int32_t rows[4];
        float pn[4];
        int pe8[4];
        for (int st = 0; st < nsteps; ++st) {
            const int bi = st / ngrp, grp = st - bi * ngrp;
            const int64_t lp = (int64_t)(b0 + 4 * bi) * 16 + 4 * c;
            if (grp == 0) {
#pragma unroll
                for (int j = 0; j < QB; ++j) acc[j] = ivf_f32x4{0.f, 0.f, 0.f, 0.f};
                // the block's position records, ahead of the next step's loads
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    rows[r] = p.perm[pos0 + lp + r];
                    pn[r] = METRIC == MQVS_METRIC_L2 ? p.pnorm[pos0 + lp + r] : 0.f;
                    pe8[r] = p.pscale[pos0 + lp + r];
                }
            }
            if (st + 1 < nsteps) load(st + 1, nxt);
#pragma unroll
            for (int u = 0; u < kIvfWin8; ++u) {
                const int64_t kw = ((int64_t)grp * kIvfWin8 + u) * 64;
                if (kw < p.dpad) {
                    const ivf_bf16x8 a0 = ivf_widen8(cur[u][0], cur[u][1]), a1 = ivf_widen8(cur[u][2], cur[u][3]);
#pragma unroll
                    for (int j = 0; j < QB; ++j) {
                        const unsigned char *qj = qp + 16 * j * qstr + 2 * kw;
                        const ivf_bf16x8 q0 = *reinterpret_cast<const ivf_bf16x8 *>(qj);
                        const ivf_bf16x8 q1 = *reinterpret_cast<const ivf_bf16x8 *>(qj + 16);
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, q0, acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, q1, acc[j], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kIvfWin8; ++u) cur[u] = nxt[u];
            if (grp != ngrp - 1) continue;
            // C: lane (l16, c) holds rows 4c..4c+3 of the block for query slot 16 j + l16
            int32_t rr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int32_t row = rows[r];
                if (row >= 0 && p.filter && !bit_test(p.filter, row)) row = -1;
                if (row >= 0 && p.exists && !bit_test(p.exists, row)) row = -1;
                rr[r] = row;
            }
#pragma unroll
            for (int j = 0; j < QB; ++j) {
                if (ent[j] < 0) continue;
                Cand out[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float raw = ldexpf(acc[j][r], -(pe8[r] + qe[j]));
                    if (!(fabsf(raw) < __builtin_inff())) raw = __builtin_nanf("");
                    if (METRIC == MQVS_METRIC_L2) raw = (s_qn[16 * j + l16] + pn[r]) - 2.0f * raw;
                    out[r].raw = rr[r] >= 0 ? raw : __builtin_nanf("");
                    out[r].row = rr[r] >= 0 ? (uint32_t)rr[r] : 0xFFFFFFFFu;
                }
                uint4 *dst = reinterpret_cast<uint4 *>(p.cand + s_base[16 * j + l16] + lp);
                dst[0] = *reinterpret_cast<const uint4 *>(&out[0]);
                dst[1] = *reinterpret_cast<const uint4 *>(&out[2]);
            }
        }
    }
}

// ---- launcher --------------------------------------------------------------

typedef void (*ivf_scan_kernel)(IvfParams);

// kern: the L2, IP and Cosine scan of one plane for 16 QB queries per item
template <int QB>
static void ivf_scan_launch(ivf_scan_kernel const (&kern)[3], const IvfParams &p, int metric, int grid,
                            hipStream_t s) {
    const size_t lds = (size_t)16 * QB * (2 * p.dpad + 16);  // the fp8 scan's tile is the bf16 scan's
    // (the caller sizes p.qg with ivf_fit_qg; a tile that does not fit is
    // refused here, never launched)
    if (ivf_scan_lds(16 * QB, p.dpad) > device_lds_bytes())
        fail(MQVS_ERR_LOGICAL, "ivf scan: " + std::to_string(16 * QB) + "-query tile of " + std::to_string(p.dpad) +
                                   " padded dimensions exceeds the workgroup's LDS");
    if (lds > 65536)  // 64-query tiles of wide rows: opt in to more than 64 KiB of LDS
        for (ivf_scan_kernel k : kern)
            MQVS_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const ivf_scan_kernel k = kern[metric == MQVS_METRIC_L2 ? 0 : metric == MQVS_METRIC_IP ? 1 : 2];
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, s, p);
}

template <int QB>
static void ivf_scan_t(const IvfParams &p, int metric, int grid, hipStream_t s) {
    static const ivf_scan_kernel bf16[3] = {k_ivf_scan<MQVS_METRIC_L2, QB>, k_ivf_scan<MQVS_METRIC_IP, QB>,
                                            k_ivf_scan<MQVS_METRIC_COSINE, QB>};
    static const ivf_scan_kernel fp8[3] = {k_ivf_scan_fp8<MQVS_METRIC_L2, QB>, k_ivf_scan_fp8<MQVS_METRIC_IP, QB>,
                                           k_ivf_scan_fp8<MQVS_METRIC_COSINE, QB>};
    ivf_scan_launch<QB>(p.plane8 ? fp8 : bf16, p, metric, grid, s);
}

void launch_ivf_scan(const IvfParams &p, int metric, int grid, hipStream_t s) {
    if (p.qg == 64)
        ivf_scan_t<4>(p, metric, grid, s);
    else if (p.qg == 32)
        ivf_scan_t<2>(p, metric, grid, s);
    else
        ivf_scan_t<1>(p, metric, grid, s);
}

}  // namespace mqvs
