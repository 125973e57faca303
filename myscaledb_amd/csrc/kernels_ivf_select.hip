// kernels_ivf_select.hip -- the index search's candidate select
// (index_kernels.h has the overview): per query, the best approximate values
// of its region of the candidate buffer.
#include "index_kernels.h"
#include "select_common.h"

namespace mqvs {

// query q's candidate region (start, length)
__device__ inline void ivf_region(const IvfRegions &g, int q, int64_t &start, int64_t &T) {
    if (g.qstart) {
        start = g.qstart[q];
        T = g.qstart[q + 1] - start;
        return;
    }
    start = (int64_t)q * g.stride;
    T = 0;
    for (int r = 0; r < g.nprobe; ++r) {
        const int64_t l = g.probes[(int64_t)q * g.nprobe + r];
        if (l >= 0 && l < g.nlist) T += g.list_off[l + 1] - g.list_off[l];
    }
}

// pair mode's stats (the plan's in the grouped mode), by the select: query
// q's [values, items, plane bytes, pairs] to stats[4 q ..] (summed by the
// final copy, k_words_to_host: 4 atomics per query on the same 4 words
// serialised the select, 26 -> 75 us at nq 1000)
__device__ inline void ivf_pair_stats(const IvfRegions &g, int q, int64_t T, bool leader) {
    if (g.qstart || !g.stats || !leader) return;
    int64_t items = 0, pairs = 0;
    for (int r = 0; r < g.nprobe; ++r) {
        const int64_t l = g.probes[(int64_t)q * g.nprobe + r];
        if (l < 0 || l >= g.nlist) continue;
        items += (g.list_off[l + 1] - g.list_off[l] + g.chunk - 1) / g.chunk;
        ++pairs;
    }
    int64_t *o = g.stats + 4 * (int64_t)q;
    o[0] = T;
    o[1] = items;
    o[2] = T * g.dpad * g.esize;
    o[3] = pairs;
}

// Per query: the R best approximate values, sorted by (key, row); at the R-th
// key the lowest rows win (every row of the region is distinct).  Writes the
// rows (for the exact re-rank) and, for first-stage-only searches, ids + the
// approximate distance.  NT threads per query; regions up to `keycap` values
// keep their keys in LDS for the four radix passes, longer ones stream them
// (4 loads in flight per thread).  The records below the R-th key and those at
// it are gathered in one pass with LDS atomics (their order does not matter:
// they are sorted); more ties at the R-th key than kTieCap, or than the
// record array has room for, fall back to a position-ordered pass for them.
constexpr int kTieCap = 64;  // <= every NT the kernel is launched with

// LARGE (R above kSortCap, num_reorder / k up to kLargeCap): the records go to
// 2 R records of global scratch per query (gscr) and are sorted there by
// global_sort (LDS runs of kSortCap, then merge passes); NT = SEL_THREADS.
template <int METRIC, int NT, bool LARGE = false>
__global__ __launch_bounds__(NT) void k_ivf_select(const Cand *cand, IvfRegions rg, int R,
                                                   int64_t *out_rows, int64_t id_offset, float *out_approx,
                                                   int keycap, uint4 *gscr, float *out_raw) {
    // pow2 >= R records (LARGE: kSortCap, the sort runs), then the key cache
    extern __shared__ __attribute__((aligned(16))) uint4 recs[];
    __shared__ uint4 ties[kTieCap];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[4];
    __shared__ int s_wave[NT / 64];
    __shared__ int s_m, s_tie;
    static_assert(!LARGE || NT == SEL_THREADS, "global_sort strides by SEL_THREADS");
    int N = 1;
    while (N < R) N <<= 1;
    uint32_t *kc = reinterpret_cast<uint32_t *>(recs + (LARGE ? kSortCap : N));
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint4 *rr = LARGE ? gscr + (int64_t)q * 2 * R : recs;  // the records (LARGE: [0, R); [R, 2R) sort scratch)
    const int mcap = LARGE ? R : N;                        // room for records below th + ties
    int64_t rs0 = 0, T = 0;
    ivf_region(rg, q, rs0, T);
    ivf_pair_stats(rg, q, T, threadIdx.x == 0);
    const Cand *c = cand + rs0;
    // A row whose approximate value is NaN (an infinite component, or
    // products that overflow to both infinities in the MFMA sum) can still
    // have a valid exact value (the fma chain of the BLAS formula stays at
    // the first infinity): before a re-rank it ranks first (key 0, below
    // every value's key) and the exact value decides; a first-stage-only
    // search has no exact value to give and leaves it out.
    const uint32_t nan_key = out_approx ? 0xFFFFFFFFu : 0u;
    auto gkey = [&](int64_t i) {
        const Cand e = c[i];
        return e.row == 0xFFFFFFFFu ? 0xFFFFFFFFu : e.raw != e.raw ? nan_key : okey<METRIC>(e.raw);
    };
    const bool cached = T <= keycap;
    if (t == 0) {
        s_m = 0;
        s_tie = 0;
    }
    uint32_t th;
    if (cached) {
        int64_t i = t;
        for (; i + 3 * NT < T; i += 4 * NT) {
            const uint32_t k0 = gkey(i), k1 = gkey(i + NT), k2 = gkey(i + 2 * NT), k3 = gkey(i + 3 * NT);
            kc[i] = k0;
            kc[i + NT] = k1;
            kc[i + 2 * NT] = k2;
            kc[i + 3 * NT] = k3;
        }
        for (; i < T; i += NT) kc[i] = gkey(i);
        __syncthreads();
        th = block_radix_select_mlp<NT>([&](int64_t j) { return kc[j]; }, T, R, hist, sh);
    } else {
        th = block_radix_select_mlp<NT>(gkey, T, R, hist, sh);
    }
    // fewer than R valid keys: every valid one; else those below th (fewer
    // than R) + the ties at th (at most kTieCap kept)
    const bool all = th == 0xFFFFFFFEu;
    auto visit = [&](int64_t i, uint32_t key) {
        if (key == 0xFFFFFFFFu) return;
        if (all || key < th) {
            const Cand e = c[i];
            const int pos = atomicAdd(&s_m, 1);
            if (pos < R) rr[pos] = make_uint4(key, e.row, __builtin_bit_cast(uint32_t, e.raw), 0u);
        } else if (key == th) {
            const Cand e = c[i];
            const int pos = atomicAdd(&s_tie, 1);
            if (pos < kTieCap) ties[pos] = make_uint4(key, e.row, __builtin_bit_cast(uint32_t, e.raw), 0u);
        }
    };
    {
        int64_t i = t;
        for (; i + 3 * NT < T; i += 4 * NT) {
            const uint32_t k0 = cached ? kc[i] : gkey(i), k1 = cached ? kc[i + NT] : gkey(i + NT),
                           k2 = cached ? kc[i + 2 * NT] : gkey(i + 2 * NT),
                           k3 = cached ? kc[i + 3 * NT] : gkey(i + 3 * NT);
            visit(i, k0);
            visit(i + NT, k1);
            visit(i + 2 * NT, k2);
            visit(i + 3 * NT, k3);
        }
        for (; i < T; i += NT) visit(i, cached ? kc[i] : gkey(i));
    }
    __syncthreads();
    const int below = min(s_m, R);
    int m = below;
    if (!all) {
        const int nt = s_tie;
        if (nt <= kTieCap && below + nt <= mcap) {
            // the ties after the records below th (kTieCap <= NT)
            if (t < nt) rr[below + t] = ties[t];
            m = below + nt;
        } else {
            // mass ties: the first R - below of them by position
            if (t == 0) s_m = below;
            __syncthreads();
            for (int64_t base = 0; base < T; base += NT) {
                const int m0 = s_m;
                if (m0 >= R) break;
                const int64_t i = base + t;
                bool flag = false;
                uint32_t key = 0xFFFFFFFFu;
                if (i < T) {
                    key = cached ? kc[i] : gkey(i);
                    flag = key == th;
                }
                const uint64_t bal = __ballot(flag);
                if (lane == 0) s_wave[wv] = __popcll(bal);
                __syncthreads();
                int off = m0;
                for (int x = 0; x < wv; ++x) off += s_wave[x];
                off += __popcll(bal & ((1ull << lane) - 1ull));
                if (flag && off < R) {
                    const Cand e = c[i];
                    rr[off] = make_uint4(key, e.row, __builtin_bit_cast(uint32_t, e.raw), 0u);
                }
                __syncthreads();
                if (t == 0) {
                    int tot = 0;
                    for (int x = 0; x < NT / 64; ++x) tot += s_wave[x];
                    s_m = min(R, m0 + tot);
                }
                __syncthreads();
            }
            m = s_m;
        }
    }
    __syncthreads();
    const uint4 *sorted = recs;
    if constexpr (LARGE) {
        sorted = global_sort(rr, rr + R, m, recs);
    } else {
    int Nm = 1;
    while (Nm < m) Nm <<= 1;
    for (int i = m + t; i < Nm; i += NT) recs[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    __syncthreads();
    // bitonic sort of recs[0, Nm) (block-wide, NT threads)
    for (int size = 2; size <= Nm; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < (Nm >> 1); i += NT) {
                const int lo = 2 * stride * (i / stride) + (i % stride);
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint4 a = recs[lo], b2 = recs[hi];
                if (rec_less(b2, a) == up) {
                    recs[lo] = b2;
                    recs[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    }
    for (int i = t; i < R; i += NT) {
        const bool ok = i < m;
        const uint4 r = ok ? sorted[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        if (out_approx) {
            out_rows[(int64_t)q * R + i] = ok ? (int64_t)r.y + id_offset : -1;
            const float raw = __builtin_bit_cast(float, r.z);
            float dist = (METRIC == MQVS_METRIC_COSINE) ? cos_dist(raw) : raw;
            if (!ok) dist = (METRIC == MQVS_METRIC_IP) ? 1.17549435e-38f : 3.40282347e+38f;
            out_approx[(int64_t)q * R + i] = dist;
        } else {
            out_rows[(int64_t)q * R + i] = ok ? (int64_t)r.y : -1;
        }
        // (the re-rank's bound pruning: the raw approximate values, NaN past the valid ones)
        if (out_raw) out_raw[(int64_t)q * R + i] = ok ? __builtin_bit_cast(float, r.z) : __builtin_nanf("");
    }
}

// Small R (the coarse quantizer: R = nprobe <= 16): one wave per query.  Each
// lane keeps its RM best (key, row) in registers over a strided slice of the
// region (8 loads in flight); the wave then pops the R smallest heads (64-bit
// min over the lanes per pop).  Order = (key, row), like k_ivf_select for a
// monotone perm.
template <int METRIC, int RM>
__global__ __launch_bounds__(256) void k_ivf_select_small(const Cand *cand, IvfRegions rg, int nq, int R,
                                                         int64_t *out_rows, int64_t id_offset, float *out_approx) {
    constexpr int U = 8;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;  // wave-uniform
    int64_t rs0 = 0, T = 0;
    ivf_region(rg, q, rs0, T);
    ivf_pair_stats(rg, q, T, lane == 0);
    const Cand *c = cand + rs0;
    uint64_t best[RM];
#pragma unroll
    for (int i = 0; i < RM; ++i) best[i] = ~0ull;
    auto insert = [&](uint64_t x) {
        if (x >= best[RM - 1]) return;
#pragma unroll
        for (int j = 0; j < RM; ++j) {
            const uint64_t lo = x < best[j] ? x : best[j];
            const uint64_t hi = x < best[j] ? best[j] : x;
            best[j] = lo;
            x = hi;
        }
    };
    for (int64_t i0 = lane; i0 < T; i0 += 64 * U) {
        uint64_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + 64 * u;
            const Cand e = i < T ? c[i] : Cand{0.f, 0xFFFFFFFFu};
            v[u] = e.row == 0xFFFFFFFFu ? ~0ull : ((uint64_t)okey<METRIC>(e.raw) << 32) | e.row;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) insert(v[u]);
    }
    // the R smallest over the wave: pop the smallest head R times
    int head = 0;
    for (int i = 0; i < R; ++i) {
        uint64_t mine = ~0ull;
#pragma unroll
        for (int j = 0; j < RM; ++j)
            if (j == head) mine = best[j];
        uint64_t m = mine;
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t y = __shfl_xor(m, o);
            m = y < m ? y : m;
        }
        if (mine == m && m != ~0ull) ++head;  // (key, row) pairs are distinct
        if (lane == 0) {
            const bool ok = m != ~0ull && (uint32_t)(m >> 32) != 0xFFFFFFFFu;
            out_rows[(int64_t)q * R + i] = ok ? (int64_t)(uint32_t)m + (out_approx ? id_offset : 0) : -1;
        }
    }
}

// ---- launcher --------------------------------------------------------------

void launch_ivf_select(const Cand *cand, const IvfRegions &rg, int nq, int R, int metric, int64_t *out_rows,
                       int64_t id_offset, float *out_approx, int64_t expect_len, hipStream_t s, uint4 *gscr,
                       float *out_raw) {
    if (R <= 16 && !out_approx && !out_raw) {
        const dim3 grid((unsigned)((nq + 3) / 4));
#define MQVS_SMALL(M, RM_) \
    hipLaunchKernelGGL((k_ivf_select_small<M, RM_>), grid, dim3(256), 0, s, cand, rg, nq, R, out_rows, id_offset, \
                       out_approx)
#define MQVS_SMALL_M(M)              \
    if (R <= 2) MQVS_SMALL(M, 2);      \
    else if (R <= 4) MQVS_SMALL(M, 4); \
    else if (R <= 8) MQVS_SMALL(M, 8); \
    else MQVS_SMALL(M, 16);
        switch (metric) {
            case MQVS_METRIC_L2: MQVS_SMALL_M(MQVS_METRIC_L2); break;
            case MQVS_METRIC_IP: MQVS_SMALL_M(MQVS_METRIC_IP); break;
            default: MQVS_SMALL_M(MQVS_METRIC_COSINE); break;
        }
#undef MQVS_SMALL_M
#undef MQVS_SMALL
        return;
    }
    const bool large = R > kSortCap;
    if (large && !gscr) fail(MQVS_ERR_LOGICAL, "ivf select: no scratch for num_reorder above 4096");
    int N = 1;
    while (N < R) N <<= 1;
    if (large) N = kSortCap;  // LDS: the sort runs
    // LDS key cache sized for the expected region length (<= 64 KiB, and
    // within the LDS left beside the records); long regions (many probed
    // lists) get 1024 threads per query
    int keycap = 1024;
    while (keycap < expect_len && keycap < 16384) keycap <<= 1;
    while (keycap > 0 && sizeof(uint4) * N + sizeof(uint32_t) * keycap > 144 * 1024) keycap >>= 1;
    const size_t lds = sizeof(uint4) * N + sizeof(uint32_t) * keycap;
    const bool wide = expect_len > 16384;
#define MQVS_SEL(M)                                                                                                 \
    do {                                                                                                            \
        if (large)                                                                                                  \
            hipLaunchKernelGGL((k_ivf_select<M, SEL_THREADS, true>), dim3(nq), dim3(SEL_THREADS), lds, s, cand,     \
                               rg, R, out_rows, id_offset, out_approx, keycap, gscr, out_raw);                  \
        else if (wide)                                                                                              \
            hipLaunchKernelGGL((k_ivf_select<M, 1024>), dim3(nq), dim3(1024), lds, s, cand, rg, R, out_rows,    \
                               id_offset, out_approx, keycap, nullptr, out_raw);                                    \
        else                                                                                                        \
            hipLaunchKernelGGL((k_ivf_select<M, SEL_THREADS>), dim3(nq), dim3(SEL_THREADS), lds, s, cand, rg, R, \
                               out_rows, id_offset, out_approx, keycap, nullptr, out_raw);                          \
    } while (0)
    switch (metric) {
        case MQVS_METRIC_L2: MQVS_SEL(MQVS_METRIC_L2); break;
        case MQVS_METRIC_IP: MQVS_SEL(MQVS_METRIC_IP); break;
        default: MQVS_SEL(MQVS_METRIC_COSINE); break;
    }
#undef MQVS_SEL
}

}  // namespace mqvs
