// kernels_ivf_pick.hip -- the index search's coarse pick (index_kernels.h has
// the overview of the path).
#include "index_kernels.h"
#include "select_common.h"

namespace mqvs {

// ---------------------------------------------------------------------------
// The coarse step's pick (index.hip): per query, from the batch probe's best
// approximate value of every group of 2^gs_log2 centroids (kernels_p4.hip,
// GRP 16 or 8), the
// exact fp32 value of each centroid of a few groups and the nprobe best.
// The group maxima are bf16 values within bq (the query's bound on |approx -
// exact|, k_query_bound) of the exact ones.
//  1. core: the T best groups (by (key, group); large T: its ties included,
//     up to Tcap), scored exactly;
//     they hold T >= nprobe centroids, so the nprobe-th best exact value of
//     the core, v, is a bound the final nprobe-th best cannot be worse than.
//  2. extras: a group outside the core can hold a centroid better than v only
//     if its maximum is within bq of v (its centroids' exact values are at
//     most maximum + bq); those groups are scored too, up to Tcap groups in
//     all.
//  3. overflow (more than Tcap groups in the core's ties or within bq of v:
//     near-ties, e.g. a query about equidistant from many centroids): every
//     group that passes is scored, in batches of Tcap taken in group order by
//     an ordered compaction, each batch merged into a running top-nprobe; the
//     query is counted in *ovf (mqvs_index_search_stats.pick_overflow).  The
//     probes stay the exact top-nprobe; only the time grows.
// Step 2 compares with the core's exact v, not with the T-th approximate
// maximum: usually no group passes (round 5 first took every group within
// 2 bq of the T-th maximum -- 8 more groups per query at nprobe 1, the pick
// 50 -> ~100 us at 39063 lists).  The probes are the exact top-nprobe of the
// centroids (in this pick's fp32 dot order).  One workgroup per query;
// Tcap <= kCoarsePickMaxT.  qn: L2 only, |q|^2 (the group values are full
// distances, the records |y|^2 - 2 ip).
//
// The group keys are staged in LDS once (up to kPickStage groups: 131072
// lists), so the four radix passes read LDS, not L2.  The exact values are
// computed a wave per kPickU centroids with float4 loads (kPickU x d/256
// independent 16-B loads per lane in flight; the pick is latency-bound, not
// bandwidth-bound: 48-160 centroids x 3 KB per query).  The nprobe best are
// placed by rank counting (M <= 256) or the LDS bitonic sort.
constexpr int kPickStage = 8192;
constexpr int kPickU = 4;
constexpr int kPickBest = kCoarsePickMaxT;  // running top-nprobe records of an overflowing pick (nprobe <= it)

template <int METRIC, bool STAGED>  // METRIC: MQVS_METRIC_L2 or kMetricIpRaw (the coarse metric)
__global__ __launch_bounds__(SEL_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_coarse_pick(const float *gmax, int64_t gld, int64_t ngroups, int T,
                                                             int Tcap, int nprobe, const float *q, int64_t qld,
                                                             const float *cent, const float *cnorm, int64_t ncent,
                                                             int d, const float *bq, const float *qnorms,
                                                             int gs_log2, int64_t *probes,
                                                             unsigned long long *ovf, int trace) {
    // (measurement build: trace = 1 prints phase timestamps of three workgroups)
    const bool tr = kDebugTuning && trace && threadIdx.x == 0 &&
                    (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2 || blockIdx.x == gridDim.x - 1);
    uint64_t ts[6] = {0, 0, 0, 0, 0, 0};
    if (tr) ts[0] = wall_clock64();
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[4];
    __shared__ int s_grp[kCoarsePickCap];
    __shared__ int s_wc[SEL_THREADS / 64];
    __shared__ int s_ng, s_valid, s_cur;
    __shared__ uint32_t s_knp;
    __shared__ uint64_t s_red[2 * (SEL_THREADS / 64)];
    // dynamic LDS: recs [pow2 >= kPickBest + GS Tcap] then (STAGED) keys
    // [ngroups], sized per launch so small pickups keep many workgroups per CU
    extern __shared__ uint4 dyn[];
    uint4 *recs = dyn;
    int NR = 1;
    const int GS = 1 << gs_log2;  // centroids per group
    while (NR < kPickBest + GS * Tcap) NR <<= 1;
    uint32_t *keys = reinterpret_cast<uint32_t *>(dyn + NR);
    const int qi = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float *row = gmax + (int64_t)qi * gld;
    // T = 1 (nprobe 1): the best (key, group) kept while staging -- one pass
    // and a block minimum instead of a second pass over the keys
    uint64_t best = ~0ull;
    if (STAGED) {
        for_each_f4(row, ngroups, [&](int64_t i, float v) {
            const uint32_t k = okey<METRIC>(v);
            keys[i] = k;
            const uint64_t pr = ((uint64_t)k << 32) | (uint64_t)(uint32_t)i;
            if (k != 0xFFFFFFFFu && pr < best) best = pr;
        });
        __syncthreads();
    }
    if (tr) ts[1] = wall_clock64();
    auto keyof = [&](int64_t i) { return STAGED ? keys[i] : okey<METRIC>(row[i]); };
    // (the core's T groups come straight from the select for T <= kSelSmallK)
    uint64_t tpair = ~0ull;  // the T-th (key << 32 | group)
    int ncore = 0;
    uint32_t th = 0xFFFFFFFEu;
    if (T == 1 && STAGED) {
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(best, off);
            best = o < best ? o : best;
        }
        if (lane == 0) s_red[wv] = best;
        __syncthreads();
        best = s_red[0];
#pragma unroll
        for (int w = 1; w < SEL_THREADS / 64; ++w) best = s_red[w] < best ? s_red[w] : best;
        if (best != ~0ull) {
            ncore = 1;
            tpair = best;
            if (t == 0) s_grp[0] = (int)(uint32_t)best;
        }
        th = tpair == ~0ull ? 0xFFFFFFFEu : (uint32_t)(tpair >> 32);
        __syncthreads();  // (s_red, s_grp)
    } else if (T <= 2) {
        ncore = block_topk_small<SEL_THREADS, 2>(keyof, ngroups, T, s_red, s_grp, &tpair);
        th = tpair == ~0ull ? 0xFFFFFFFEu : (uint32_t)(tpair >> 32);
    } else if (T <= 4) {
        ncore = block_topk_small<SEL_THREADS, 4>(keyof, ngroups, T, s_red, s_grp, &tpair);
        th = tpair == ~0ull ? 0xFFFFFFFEu : (uint32_t)(tpair >> 32);
    } else if (T <= kSelSmallK) {
        ncore = block_topk_small(keyof, ngroups, T, s_red, s_grp, &tpair);
        th = tpair == ~0ull ? 0xFFFFFFFEu : (uint32_t)(tpair >> 32);
    } else {
        th = block_radix_select_mlp(keyof, ngroups, T, hist, sh);
    }
    if (t == 0) {
        s_ng = ncore;
        s_valid = 0;
        s_knp = 0xFFFFFFFFu;
    }
    __syncthreads();
    if (tr) ts[2] = wall_clock64();
    // the groups whose key passes take(key, group), appended to s_grp (up to Tcap)
    auto collect = [&](auto take) {
        for (int64_t i = t; i < ngroups; i += SEL_THREADS) {
            const uint32_t k = keyof(i);
            if (k == 0xFFFFFFFFu || !take(k, i)) continue;
            const int slot = atomicAdd(&s_ng, 1);
            if (slot < Tcap) s_grp[slot] = (int)i;
        }
        __syncthreads();
    };
    // exact values of centroids c in [cb, ce) (GS per taken group) into
    // recs[ro + c]: wave wv scores centroids c0 .. c0 + kPickU - 1, lanes over
    // float4 columns (scalar columns when d or the rows are not 16-B aligned)
    const float *qv = q + (int64_t)qi * qld;
    const bool v4 = (d & 3) == 0 && (((uintptr_t)cent | (uintptr_t)qv) & 15) == 0;
    auto score = [&](int cb, int ce, int ro) {
        for (int c0 = cb + wv * kPickU; c0 < ce; c0 += (SEL_THREADS / 64) * kPickU) {
            int64_t r[kPickU];
            float dot[kPickU];
#pragma unroll
            for (int u = 0; u < kPickU; ++u) {
                const int c = c0 + u;
                r[u] = c < ce ? ((int64_t)s_grp[c >> gs_log2] << gs_log2) + (c & (GS - 1)) : ncent;
                if (r[u] >= ncent) r[u] = -1;
                dot[u] = 0.f;
            }
            if (v4) {
                const float4 *q4 = reinterpret_cast<const float4 *>(qv);
                // three column steps per round: 3 kPickU independent 16-B loads
                // per lane in flight (d = 768 is one round)
                const int n4 = d >> 2;
                for (int j0 = lane; j0 < n4; j0 += 3 * 64) {
                    float4 x[3], y[3][kPickU];
#pragma unroll
                    for (int tt = 0; tt < 3; ++tt) {
                        const int j = j0 + 64 * tt;
                        const bool in = j < n4;
                        x[tt] = in ? q4[j] : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int u = 0; u < kPickU; ++u)
                            y[tt][u] = in && r[u] >= 0 ? reinterpret_cast<const float4 *>(cent + r[u] * d)[j]
                                                       : float4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int tt = 0; tt < 3; ++tt)
#pragma unroll
                        for (int u = 0; u < kPickU; ++u) {
                            dot[u] = fmaf(x[tt].x, y[tt][u].x, dot[u]);
                            dot[u] = fmaf(x[tt].y, y[tt][u].y, dot[u]);
                            dot[u] = fmaf(x[tt].z, y[tt][u].z, dot[u]);
                            dot[u] = fmaf(x[tt].w, y[tt][u].w, dot[u]);
                        }
                }
            } else {
                for (int e = lane; e < d; e += 64) {
                    const float x = qv[e];
#pragma unroll
                    for (int u = 0; u < kPickU; ++u)
                        if (r[u] >= 0) dot[u] = fmaf(x, cent[r[u] * d + e], dot[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kPickU; ++u) {
                float v = dot[u];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                dot[u] = v;
            }
            if (lane < kPickU) {
                float dv = dot[0];
                int64_t rv = r[0];
#pragma unroll
                for (int u = 1; u < kPickU; ++u)
                    if (lane == u) {
                        dv = dot[u];
                        rv = r[u];
                    }
                const int c = c0 + lane;
                if (c < ce) {
                    uint32_t key = 0xFFFFFFFFu;
                    if (rv >= 0) key = okey<METRIC>(METRIC == MQVS_METRIC_L2 ? cnorm[rv] - 2.0f * dv : dv);
                    recs[ro + c] = uint4{key, (uint32_t)(rv >= 0 ? rv : 0xFFFFFFFFu), 0u, 0u};
                    if (key != 0xFFFFFFFFu) atomicAdd(&s_valid, 1);
                }
            }
        }
        __syncthreads();
    };
    // 1. core: the T best (key, group) pairs (large T: the groups better than
    // the T-th key, then its ties)
    if (T > kSelSmallK) {
        collect([&](uint32_t k, int64_t) { return th == 0xFFFFFFFEu || k < th; });
        if (th != 0xFFFFFFFEu) collect([&](uint32_t k, int64_t) { return k == th; });
        tpair = th == 0xFFFFFFFEu ? ~0ull : ((uint64_t)th << 32) | 0xFFFFFFFFull;  // (every tie is in)
    }
    const int ng0 = min(s_ng, Tcap);
    // (a core with more ties than Tcap groups: overflow)
    bool over = s_ng > Tcap;
    score(0, GS * ng0, 0);
    if (tr) ts[3] = wall_clock64();
    int ng = ng0;
    uint32_t kx = th;  // every group that can hold a top-nprobe centroid has key <= max(kx, th)
    // 2. extras (needs the bound and a full core; fewer than T valid groups:
    // every group is in the core already).  The collect counts every group
    // that passes, so a working set that cannot hold them shows as s_ng > Tcap.
    if (bq && tpair != ~0ull) {
        const int M0 = GS * ng0;
        for (int c = t; c < M0; c += SEL_THREADS) {
            const uint4 e = recs[c];
            if (e.x == 0xFFFFFFFFu) continue;
            int rank = 0;
            for (int o = 0; o < M0; ++o) rank += rec_less(recs[o], e) ? 1 : 0;
            if (rank == nprobe - 1) s_knp = e.x;
        }
        __syncthreads();
        if (s_knp != 0xFFFFFFFFu) {
            // the approximate maximum a group needs: v -/+ bq (rounding slack
            // as widen's), v a full distance for L2
            float v = okey_value<METRIC>(s_knp);
            if (METRIC == MQVS_METRIC_L2) v = qnorms[qi] + v;
            const float b = bq[qi];
            float w;
            if (METRIC == MQVS_METRIC_L2) {
                w = v + b;
                w = w + fabsf(w) * 2.4e-7f + 1e-30f;
            } else {
                w = v - b;
                w = w - fabsf(w) * 2.4e-7f - 1e-30f;
            }
            kx = w == w ? okey<METRIC>(w) : th;
        } else {
            // fewer than nprobe valid centroids in the core: every group
            // within 2 bq of the T-th maximum
            const float w = widen<METRIC>(okey_value<METRIC>(th), bq[qi]);
            kx = w == w ? okey<METRIC>(w) : th;
        }
        if (kx >= th && !over) {
            collect([&](uint32_t k, int64_t i) {
                return k <= kx && (((uint64_t)k << 32) | (uint64_t)(uint32_t)i) > tpair;
            });
            over = s_ng > Tcap;
            ng = min(s_ng, Tcap);
            if (!over && ng > ng0) score(M0, GS * ng, 0);
        }
    }
    if (over) {
        // 3. every group with key <= max(kx, th), Tcap groups at a time in
        // group order; recs[0, nprobe) keeps the best so far (sorted), the
        // batch's records follow at kPickBest
        if (t == 0 && ovf) atomicAdd(ovf, 1ull);
        const uint32_t kall = kx > th ? kx : th;
        for (int c = t; c < kPickBest; c += SEL_THREADS) recs[c] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        int64_t cursor = 0;
        while (cursor < ngroups) {
            // ordered compaction of the next Tcap passing groups from `cursor`
            int nb = 0;
            int64_t i0 = cursor;
            while (i0 < ngroups && nb < Tcap) {
                const int64_t i = i0 + t;
                bool pass = false;
                if (i < ngroups) {
                    const uint32_t kk = keyof(i);
                    pass = kk != 0xFFFFFFFFu && kk <= kall;
                }
                const uint64_t bal = __ballot(pass);
                if (lane == 0) s_wc[wv] = __popcll(bal);
                __syncthreads();
                int before = 0, tot = 0;
                for (int x = 0; x < SEL_THREADS / 64; ++x) {
                    before += x < wv ? s_wc[x] : 0;
                    tot += s_wc[x];
                }
                const int pos = nb + before + __popcll(bal & ((1ull << lane) - 1ull));
                if (pass && pos < Tcap) s_grp[pos] = (int)i;
                if (pass && pos == Tcap - 1) s_cur = (int)(i + 1);
                __syncthreads();
                if (nb + tot >= Tcap) {
                    i0 = s_cur;
                    nb = Tcap;
                } else {
                    nb += tot;
                    i0 += SEL_THREADS;
                }
                __syncthreads();  // (s_wc, s_cur reused)
            }
            cursor = i0;
            if (nb == 0) break;
            score(0, GS * nb, kPickBest);
            int N = 1;
            while (N < kPickBest + GS * nb) N <<= 1;
            for (int c = kPickBest + GS * nb + t; c < N; c += SEL_THREADS)
                recs[c] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            __syncthreads();
            block_bitonic_sort(recs, N);
            for (int c = nprobe + t; c < kPickBest; c += SEL_THREADS)
                recs[c] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            __syncthreads();
        }
        for (int j = t; j < nprobe; j += SEL_THREADS) {
            const uint4 e = recs[j];
            probes[(int64_t)qi * nprobe + j] = e.x == 0xFFFFFFFFu ? -1 : (int64_t)e.y;
        }
        return;
    }
    const int M = GS * ng;
    __syncthreads();
    if (tr) ts[4] = wall_clock64();
    auto trace_out = [&]() {
        if (tr)
            printf("pick q %d ng0 %d ng %d stage %llu select %llu core %llu extras %llu place %llu (x10ns)\n", qi,
                   ng0, ng, (unsigned long long)(ts[1] - ts[0]), (unsigned long long)(ts[2] - ts[1]),
                   (unsigned long long)(ts[3] - ts[2]), (unsigned long long)(ts[4] - ts[3]),
                   (unsigned long long)(wall_clock64() - ts[4]));
    };
    const int nvalid = s_valid;
    if (M <= 256) {
        // rank counting: valid records are unique (key, centroid), so each
        // lands on its own rank; the invalid ones are not placed
        for (int c = t; c < M; c += SEL_THREADS) {
            const uint4 e = recs[c];
            if (e.x == 0xFFFFFFFFu) continue;
            int rank = 0;
            for (int o = 0; o < M; ++o) rank += rec_less(recs[o], e) ? 1 : 0;
            if (rank < nprobe) probes[(int64_t)qi * nprobe + rank] = (int64_t)e.y;
        }
        for (int j = nvalid + t; j < nprobe; j += SEL_THREADS) probes[(int64_t)qi * nprobe + j] = -1;
        trace_out();
        return;
    }
    int N = 1;
    while (N < M) N <<= 1;
    for (int c = M + t; c < N; c += SEL_THREADS) recs[c] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    __syncthreads();
    block_bitonic_sort(recs, N);
    for (int j = t; j < nprobe; j += SEL_THREADS) {
        const uint4 e = j < M ? recs[j] : uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
        probes[(int64_t)qi * nprobe + j] = e.x == 0xFFFFFFFFu ? -1 : (int64_t)e.y;
    }
    trace_out();
}

void launch_coarse_pick(const float *gmax, int64_t gld, int64_t ngroups, int T, int nprobe, int metric,
                        const float *q, int64_t qld, const float *cent, const float *cnorm, int64_t ncent, int d,
                        const float *bq, const float *qnorms, int gs_log2, int nq, int64_t *probes,
                        unsigned long long *ovf, hipStream_t s) {
    if (nq <= 0) return;
    if (T > kCoarsePickMaxT || nprobe > kPickBest) fail(MQVS_ERR_LOGICAL, "coarse pick: nprobe above its cap");
    // room for the groups within the bound of the core's nprobe-th value
    // (near-ties): as many as a core of nprobe + 2 groups had (a smaller core
    // leaves more of the near groups to the extras); more are the overflow
    // path's (exact, batched)
    const int Tcap = std::min(kCoarsePickCap, std::max(T, nprobe + 2) + std::max(std::max(T, nprobe + 2), 8));
    const int trace = tune_int("MQVS_PICK_TRACE", 0);
#define MQVS_PICK(M, ST)                                                                                         \
    hipLaunchKernelGGL((k_coarse_pick<M, ST>), dim3(nq), dim3(SEL_THREADS), lds, s, gmax, gld, ngroups, T, Tcap, \
                       nprobe, q, qld, cent, cnorm, ncent, d, bq, qnorms, gs_log2, probes, ovf, trace)
    const bool staged = ngroups <= kPickStage;
    size_t nr = 1;
    while (nr < kPickBest + ((size_t)1 << gs_log2) * Tcap) nr <<= 1;
    const size_t lds = nr * sizeof(uint4) + (staged ? sizeof(uint32_t) * (size_t)ngroups : 0);
    if (metric == MQVS_METRIC_L2) {
        if (staged) MQVS_PICK(MQVS_METRIC_L2, true); else MQVS_PICK(MQVS_METRIC_L2, false);
    } else {
        if (staged) MQVS_PICK(kMetricIpRaw, true); else MQVS_PICK(kMetricIpRaw, false);
    }
#undef MQVS_PICK
}

}  // namespace mqvs
