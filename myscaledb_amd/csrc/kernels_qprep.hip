// kernels_qprep.hip -- query preparation: the stored query, |q|^2 for the BLAS
// branch, and for cosine the chain of re-normalised variants.
#include "flat_kernels.h"

namespace mqvs {

// Query preparation, one wave per query.  L2/IP: variant 0 = the query,
// qnorm = |q|^2 (BLAS branch).  Cosine: the reference normalises the SAME
// query object once per searched granule chunk (VIWithDataPart.h:358 on the
// dataset shared across chunks, MergeTreeVSManager.cpp:1279-1292,1473-1486),
// so chunk ordinal c uses normalize^(c+1)(q).  Variants are generated until a
// repeat: variants [0, mu) are the transient, [mu, mu+lam) the cycle.
//
// The sums are sequential fp32 (product rounded, then added: the order of
// VectorDataset::normalize / fvec_norm_L2sqr), a 768-long dependent chain per
// normalisation.  Lane l holds elements l + 64 j in registers (J slots); the
// chain walks them with v_readlane into the wave-uniform accumulator, so it
// costs one readlane + one add per element instead of an LDS round trip.
// J = 0: generic d (elements in LDS, lane 0 walks them).
// sum_{i<d} x_i^2, sequential fp32 (x_i held by lane i % 64, slot i / 64).
// Padding elements (i >= d) hold 0 and add +0.0f, which leaves the
// non-negative running sum bit-identical, so every slot walks all 64 lanes
// without branches; readlanes go 16 at a time ahead of their adds.
template <int J>
__device__ __forceinline__ float seq_sq_sum(const float (&x)[J], int d) {
    (void)d;
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < J; ++u) {
        const int sq = __builtin_bit_cast(int, x[u] * x[u]);
#pragma unroll
        for (int l0 = 0; l0 < 64; l0 += 16) {
            float t[16];
#pragma unroll
            for (int l = 0; l < 16; ++l) t[l] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(sq, l0 + l));
#pragma unroll
            for (int l = 0; l < 16; ++l) acc = acc + t[l];
        }
    }
    return acc;
}

// The same sum through LDS: the rounded products are stored once, and every
// lane walks them in order from 16-B broadcast reads (4 elements per read;
// the reads run ahead of the dependent adds).  Same order, same bits.
template <int J>
__device__ __forceinline__ float seq_sq_sum_lds(const float (&x)[J], float *prod) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < J; ++u) prod[lane + 64 * u] = x[u] * x[u];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the stores landed (one wave)
    __builtin_amdgcn_wave_barrier();
    float acc = 0.0f;
    const float4 *p4 = reinterpret_cast<const float4 *>(prod);
#pragma unroll 8
    for (int i = 0; i < 16 * J; ++i) {
        const float4 v = p4[i];
        acc = acc + v.x;
        acc = acc + v.y;
        acc = acc + v.z;
        acc = acc + v.w;
    }
    __builtin_amdgcn_wave_barrier();  // (the next step rewrites prod)
    return acc;
}

// The same walk software-pipelined: the 16-B reads of block b + 1 are issued
// before the adds of block b, so the dependent add chain never waits on LDS
// latency (the plain loop above issues a block's reads only after the previous
// block's adds).  Same order, same bits.
template <int J>
__device__ __forceinline__ float seq_sq_sum_lds_pipe(const float (&x)[J], float *prod) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < J; ++u) prod[lane + 64 * u] = x[u] * x[u];
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    constexpr int B = 4;              // float4 reads per block
    constexpr int NB = 16 * J / B;    // blocks
    const float4 *p4 = reinterpret_cast<const float4 *>(prod);
    float4 cur[B], nxt[B];
#pragma unroll
    for (int i = 0; i < B; ++i) cur[i] = p4[i];
    float acc = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB) {
#pragma unroll
            for (int i = 0; i < B; ++i) nxt[i] = p4[(b + 1) * B + i];
        }
#pragma unroll
        for (int i = 0; i < B; ++i) {
            acc = acc + cur[i].x;
            acc = acc + cur[i].y;
            acc = acc + cur[i].z;
            acc = acc + cur[i].w;
        }
#pragma unroll
        for (int i = 0; i < B; ++i) cur[i] = nxt[i];
    }
    __builtin_amdgcn_wave_barrier();
    return acc;
}

// The same sum from registers: the rounded products go through LDS once and
// lane L < 8 loads elements [8 J L, 8 J (L + 1)) into its registers (2 J
// 16-B reads, all issued up front); then eight phases of 8 J dependent adds,
// phase L continuing the running sum of phase L - 1 (readlane broadcast) with
// lane L's elements.  The add chain never waits on LDS (the walk above
// re-reads LDS for every 4 elements); same order, same bits.
template <int J>
__device__ __forceinline__ float seq_sq_sum_lanes(const float (&x)[J], float *prod) {
    constexpr int NL = 8, PL = 8 * J;  // lanes, elements per lane (64 J = NL PL)
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < J; ++u) prod[lane + 64 * u] = x[u] * x[u];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the stores landed (one wave)
    __builtin_amdgcn_wave_barrier();
    const float4 *p4 = reinterpret_cast<const float4 *>(prod + (lane < NL ? lane : 0) * PL);
    float v[PL];
#pragma unroll
    for (int j = 0; j < PL / 4; ++j) {
        const float4 t = p4[j];
        v[4 * j] = t.x;
        v[4 * j + 1] = t.y;
        v[4 * j + 2] = t.z;
        v[4 * j + 3] = t.w;
    }
    // (every read issued before the first add: left to itself the compiler
    // sinks the reads into phase 0, two at a time, each pair waited for)
    __builtin_amdgcn_sched_barrier(0);
    float acc = 0.0f;
#pragma unroll
    for (int L = 0; L < NL; ++L) {
#pragma unroll
        for (int i = 0; i < PL; ++i) acc = acc + v[i];
        acc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, acc), L));
    }
    __builtin_amdgcn_wave_barrier();  // (the next step rewrites prod)
    return acc;
}

// J > 0: d <= 64 J, the query in registers.
// phase 0: everything.  Cosine searches whose first consumers need only
// variant 0 split the work: phase 1 writes variant 0 (and |q|^2 = 0); phase 2,
// launched after it (on a side stream, concurrent with the coarse step and the
// list scan), walks the rest of the chain -- it compares against the stored
// variant 0 but does not rewrite it -- and writes mu, lambda and the status.
// SUMV: 0 = readlane walk (seq_sq_sum), 1 = LDS broadcast walk
// (seq_sq_sum_lds: 39.0 -> 35.5 us at nq 1, 72.5 -> 65.7 us at nq 1000 for
// d = 768), 2 = that walk software-pipelined (slower: 45 us), 3 = register
// phases (seq_sq_sum_lanes, the launcher's); bit-identical tables,
// tools/qprep_sum_ab.hip, profiles/r05/qprep_sum_ab.jsonl
constexpr int kLaneSigMax = 32;  // variants whose per-lane signatures fit LDS (33 x 256 B)
// qdelta (may be null; cosine): per query an upper bound on the largest
// |x_v - x_0| over the variants the chain produces (the index re-rank's bound
// pruning compares exact values of variant x_v with variant-0 approximations):
// per lane the largest fp64 partial sum of squares over the variants, summed
// over the lanes (a sum of maxima bounds the maximum of sums), rounded up.
template <int J, int SUMV = 0, bool LANESIG = false>
__global__ __launch_bounds__(64) void k_query_prep(const float *q, int nq, int d, int metric, int blas, float *qvars,
                                                   int maxv, float *qnorms, int *qmu, int *qlam, int *status,
                                                   int phase, float *qdelta) {
    __shared__ __attribute__((aligned(16))) float prod[SUMV ? 64 * J : 1];
    auto sqsum = [&](const float(&xx)[J]) -> float {
        if constexpr (SUMV == 3)
            return seq_sq_sum_lanes<J>(xx, prod);
        else if constexpr (SUMV == 2)
            return seq_sq_sum_lds_pipe<J>(xx, prod);
        else if constexpr (SUMV == 1)
            return seq_sq_sum_lds<J>(xx, prod);
        else
            return seq_sq_sum<J>(xx, 0);
    };
    const int j = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t qs = (int64_t)((d + 31) / 32 * 32);
    const float *src = q + (int64_t)j * d;
    float *v0 = qvars + (int64_t)j * maxv * qs;
    float x[J];
#pragma unroll
    for (int u = 0; u < J; ++u) {
        const int i = lane + 64 * u;
        x[u] = i < d ? src[i] : 0.0f;
    }
    if (metric != MQVS_METRIC_COSINE) {
        if (phase == 2) return;
        if (qdelta && lane == 0) qdelta[j] = 0.0f;
        // (columns d .. qs: zeros; the table is not cleared beforehand and
        // the padded readers take them)
#pragma unroll
        for (int u = 0; u < J; ++u)
            if (lane + 64 * u < qs) v0[lane + 64 * u] = x[u];
        const float sum = blas ? sqsum(x) : 0.0f;
        if (lane == 0) {
            if (qnorms) qnorms[j] = sum;
            qmu[j] = 0;
            qlam[j] = 1;
        }
        return;
    }
    const float eps = 1.1920929e-07f;
    // variants 0..maxv-1 are stored; normalisation maxv is only compared, so a
    // fixed point reached at the last stored variant is still detected.  A
    // repeat is found by a signature of each variant; only a signature match
    // is confirmed element by element.  LANESIG (maxv <= kLaneSigMax): a 32-bit
    // hash per lane, kept per variant in LDS and matched with one vote (no
    // cross-lane reduction: 0.3 -> ~0.05 us per normalisation); else one 64-bit
    // hash per variant, wave-reduced.
    extern __shared__ uint64_t sig[];  // LANESIG: [maxv + 1][64] uint32; else maxv + 1 uint64
    uint32_t *lsig = reinterpret_cast<uint32_t *>(sig);
    float x0[J];
    double dl = 0.0;
    auto put_delta = [&]() {
        if (!qdelta) return;
        double t = dl;
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0) qdelta[j] = (float)(sqrt(t) * (1.0 + 1e-6)) + 1e-30f;
    };
    for (int v = 0; v <= maxv; ++v) {
        const float sum = sqsum(x);
        if (!(sum < eps)) {
            const float sr = sqrtf(sum);
#pragma unroll
            for (int u = 0; u < J; ++u) x[u] = x[u] / sr;
        }
        if (qdelta) {
            if (v == 0) {
#pragma unroll
                for (int u = 0; u < J; ++u) x0[u] = x[u];
            } else {
                double ss = 0.0;
#pragma unroll
                for (int u = 0; u < J; ++u) {
                    const double e = (double)x[u] - (double)x0[u];
                    ss += e * e;
                }
                dl = ss > dl ? ss : dl;
            }
        }
        if (v < maxv && (phase != 2 || v > 0)) {
            float *cur = v0 + (int64_t)v * qs;
            if (64 * J == qs) {
                // every slot in range: one address, immediate offsets (the
                // per-slot predicate below makes the compiler rebuild the
                // address before each store and wait for the previous store:
                // ~1 us per normalisation)
#pragma unroll
                for (int u = 0; u < J; ++u) cur[lane + 64 * u] = x[u];
            } else {
#pragma unroll
                for (int u = 0; u < J; ++u)
                    if (lane + 64 * u < qs) cur[lane + 64 * u] = x[u];  // (x = 0 past d)
            }
        }
        if (phase == 1) {
            if (lane == 0 && qnorms) qnorms[j] = 0.0f;
            return;
        }
        uint64_t h = 0;
        uint32_t hl = 0x811C9DC5u;
        if constexpr (LANESIG) {
#pragma unroll
            for (int u = 0; u < J; ++u) {
                const uint32_t b = __builtin_bit_cast(uint32_t, x[u]);
                hl = ((hl << 5) | (hl >> 27)) ^ (b + 0x9E3779B9u * (uint32_t)(u + 1));
            }
            if (v < maxv) lsig[v * 64 + lane] = hl;
            __builtin_amdgcn_wave_barrier();  // (one wave: its LDS ops complete in order)
        } else {
#pragma unroll
            for (int u = 0; u < J; ++u) {
                const uint64_t b = __builtin_bit_cast(uint32_t, x[u]);
                h += (b + 0x9E3779B97F4A7C15ull * (uint64_t)(u + 1)) * (b | 1ull) ^ (b << 29);
            }
            for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
            if (v < maxv && lane == 0) sig[v] = h;
            __syncthreads();
        }
        for (int u = 0; u < v; ++u) {
            if constexpr (LANESIG) {
                if (!__all(lsig[u * 64 + lane] == hl)) continue;
            } else if (sig[u] != h) {
                continue;
            }
            const float *o = v0 + (int64_t)u * qs;
            bool eq = true;
#pragma unroll
            for (int w = 0; w < J; ++w)
                if (lane + 64 * w < d)
                    eq = eq && __builtin_bit_cast(uint32_t, o[lane + 64 * w]) == __builtin_bit_cast(uint32_t, x[w]);
            if (__all(eq)) {
                if (lane == 0) {
                    qmu[j] = u;
                    qlam[j] = v - u;
                    if (qnorms) qnorms[j] = 0.0f;
                }
                // the variants past the chain are never selected, but the bf16
                // plane and the bound read every stored one: zeros (the table
                // is not cleared beforehand)
                // (16-B stores: variants are 128-B aligned, qs a multiple of 32)
                float4 *z = reinterpret_cast<float4 *>(v0 + (int64_t)v * qs);
                const int64_t n4 = (int64_t)(maxv - v) * qs / 4;
                for (int64_t i = lane; i < n4; i += 64) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                put_delta();
                return;
            }
        }
    }
    put_delta();
    if (lane == 0) {
        // no repeat within maxv + 1 normalisations: variants 0..maxv-1 are
        // exact, later chunk ordinals are not (the host fails the search if
        // the part has that many searched chunks)
        atomicOr(status, 1);
        qmu[j] = maxv - 1;
        qlam[j] = 1;
        if (qnorms) qnorms[j] = 0.0f;
    }
}

// generic d: elements in LDS, lane 0 walks the sequential sums
// (phase 1 makes the whole chain here; phase 2 -- launched after it, with the
// qdelta buffer the re-rank's bound pruning reads -- only measures the spread
// of the variants phase 1 stored)
__global__ __launch_bounds__(64) void k_query_prep_lds(const float *q, int nq, int d, int metric, int blas,
                                                       float *qvars, int maxv, float *qnorms, int *qmu, int *qlam,
                                                       int *status, int phase, float *qdelta) {
    extern __shared__ __attribute__((aligned(16))) float qbuf[];
    const int j = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t qs = (int64_t)((d + 31) / 32 * 32);
    const float *src = q + (int64_t)j * d;
    float *v0 = qvars + (int64_t)j * maxv * qs;
    // qdelta as k_query_prep's, from the stored variants [1, nv)
    auto put_delta = [&](int nv) {
        if (!qdelta) return;
        double dl = 0.0;
        for (int v = 1; v < nv; ++v) {
            double ss = 0.0;
            for (int i = lane; i < d; i += 64) {
                const double e = (double)v0[(int64_t)v * qs + i] - (double)v0[i];
                ss += e * e;
            }
            dl = ss > dl ? ss : dl;
        }
        for (int off = 32; off > 0; off >>= 1) dl += __shfl_xor(dl, off);
        if (lane == 0) qdelta[j] = (float)(sqrt(dl) * (1.0 + 1e-6)) + 1e-30f;
    };
    if (phase == 2) {
        // the stored variants are [0, mu + lambda) (all maxv when the chain
        // did not repeat: phase 1 then left mu = maxv - 1, lambda = 1)
        if (metric == MQVS_METRIC_COSINE) {
            const int mu = qmu[j], lam = qlam[j];
            put_delta((lam >= 1 && mu >= 0 && mu + lam <= maxv) ? mu + lam : maxv);
        } else if (qdelta && lane == 0) {
            qdelta[j] = 0.0f;
        }
        return;
    }
    for (int i = lane; i < d; i += 64) qbuf[i] = src[i];
    __syncthreads();
    auto seqsum = [&]() -> float {
        if (lane == 0) {
            float s = 0.0f;
#pragma unroll 8
            for (int i = 0; i < d; ++i) s = s + qbuf[i] * qbuf[i];
            qbuf[qs] = s;
        }
        __syncthreads();
        const float r = qbuf[qs];
        __syncthreads();
        return r;
    };
    if (metric != MQVS_METRIC_COSINE) {
        for (int i = lane; i < qs; i += 64) v0[i] = i < d ? qbuf[i] : 0.0f;
        const float sum = blas ? seqsum() : 0.0f;
        if (qdelta && lane == 0) qdelta[j] = 0.0f;
        if (lane == 0) {
            if (qnorms) qnorms[j] = sum;
            qmu[j] = 0;
            qlam[j] = 1;
        }
        return;
    }
    const float eps = 1.1920929e-07f;
    for (int v = 0; v <= maxv; ++v) {
        float *cur = v < maxv ? v0 + (int64_t)v * qs : nullptr;
        const float sum = seqsum();
        if (sum < eps) {
            if (cur)
                for (int i = lane; i < d; i += 64) cur[i] = qbuf[i];
        } else {
            const float s = sqrtf(sum);
            for (int i = lane; i < d; i += 64) {
                const float x = qbuf[i] / s;
                if (cur) cur[i] = x;
                qbuf[i] = x;
            }
        }
        if (cur)
            for (int i = d + lane; i < qs; i += 64) cur[i] = 0.0f;  // (padding columns)
        __syncthreads();
        for (int u = 0; u < v; ++u) {
            const float *o = v0 + (int64_t)u * qs;
            bool eq = true;
            for (int i = lane; i < d; i += 64)
                eq = eq && __builtin_bit_cast(uint32_t, o[i]) == __builtin_bit_cast(uint32_t, qbuf[i]);
            if (__all(eq)) {
                if (lane == 0) {
                    qmu[j] = u;
                    qlam[j] = v - u;
                    if (qnorms) qnorms[j] = 0.0f;
                }
                for (int w = v; w < maxv; ++w)  // (unused variants: zeros)
                    for (int i = lane; i < qs; i += 64) v0[(int64_t)w * qs + i] = 0.0f;
                put_delta(v);
                return;
            }
        }
    }
    put_delta(maxv);
    if (lane == 0) {
        atomicOr(status, 1);
        qmu[j] = maxv - 1;
        qlam[j] = 1;
        if (qnorms) qnorms[j] = 0.0f;
    }
}

void launch_query_prep(const float *q, int nq, int d, int metric, bool blas, float *qvars, int maxv,
                       float *qnorms, int *qmu, int *qlam, int *status, hipStream_t s, int phase, float *qdelta) {
    if (metric != MQVS_METRIC_COSINE) maxv = 1;
    const size_t lds = (size_t)((d + 31) / 32 * 32 + 4) * sizeof(float);
    const bool lanesig = maxv <= kLaneSigMax;
    const size_t sig = lanesig ? (size_t)(maxv + 1) * 64 * sizeof(uint32_t) : (size_t)(maxv + 1) * sizeof(uint64_t);
#define MQVS_QP(J)                                                                                                   \
    do {                                                                                                             \
        if (lanesig)                                                                                                 \
            hipLaunchKernelGGL((k_query_prep<J, 3, true>), dim3(nq), dim3(64), sig, s, q, nq, d, metric, blas ? 1 : 0, \
                               qvars, maxv, qnorms, qmu, qlam, status, phase, qdelta);                               \
        else                                                                                                         \
            hipLaunchKernelGGL((k_query_prep<J, 3, false>), dim3(nq), dim3(64), sig, s, q, nq, d, metric,             \
                               blas ? 1 : 0, qvars, maxv, qnorms, qmu, qlam, status, phase, qdelta);                 \
    } while (0)
    if (d <= 128)
        MQVS_QP(2);
    else if (d <= 256)
        MQVS_QP(4);
    else if (d <= 512)
        MQVS_QP(8);
    else if (d <= 768)
        MQVS_QP(12);
    else if (d <= 1024)
        MQVS_QP(16);
    else if (d <= 1536)
        MQVS_QP(24);
    else
        hipLaunchKernelGGL(k_query_prep_lds, dim3(nq), dim3(64), lds, s, q, nq, d, metric, blas ? 1 : 0, qvars, maxv,
                           qnorms, qmu, qlam, status, phase, qdelta);
#undef MQVS_QP
}

}  // namespace mqvs
