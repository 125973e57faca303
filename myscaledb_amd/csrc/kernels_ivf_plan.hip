// kernels_ivf_plan.hip -- the index search's plan (index_kernels.h has the
// overview): the (query, probe) pairs grouped by list and cut into the scan's
// work items, and the probes of the dense case.
#include "index_kernels.h"

namespace mqvs {

constexpr int kPlanThreads = 1024;

// Exclusive scan of `n` int64 values produced by val(i) into out(i, prefix);
// returns the total.  One workgroup of kPlanThreads; each thread owns a
// contiguous run, run sums are scanned in LDS.
template <class Val, class Out>
__device__ int64_t block_exclusive_scan(int64_t n, Val val, Out out, int64_t *sh) {
    const int t = threadIdx.x;
    const int64_t per = (n + kPlanThreads - 1) / kPlanThreads;
    const int64_t b = t * per, e = min(n, b + per);
    int64_t s = 0;
    for (int64_t i = b; i < e; ++i) s += val(i);
    // block prefix of the run sums: wave scans, then the 16 wave totals
    const int lane = t & 63, wv = t >> 6;
    int64_t inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    if (t == 0) {
        int64_t acc = 0;
        for (int w = 0; w < kPlanThreads / 64; ++w) {
            const int64_t v = sh[w];
            sh[w] = acc;
            acc += v;
        }
        sh[kPlanThreads] = acc;
    }
    __syncthreads();
    int64_t run = sh[wv] + inc - s;
    for (int64_t i = b; i < e; ++i) {
        const int64_t v = val(i);
        out(i, run);
        run += v;
    }
    const int64_t total = sh[kPlanThreads];
    __syncthreads();
    return total;
}

// Plan, in four launches (the pairs are spread over the grid; only the two
// prefix sums run in a single workgroup):
//   count    lcount[l] = pairs probing list l
//   lists    exclusive scans over the lists: lstart (pairs), work items
//   scatter  pairs grouped by list; per query, probe offsets inside its region
//   queries  exclusive scan of the query regions (qstart)
__global__ __launch_bounds__(256) void k_plan_count(IvfParams p) {
    const int64_t E = (int64_t)p.nq * p.nprobe;
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        const int64_t l = p.probes[e];
        if (l >= 0 && l < p.nlist) atomicAdd(&p.lcount[l], 1);
    }
}

// Workgroup b owns kPlanBlk lists: their (pair count, length) are staged in
// LDS by coalesced loads, then thread t walks lists [kPlanPer t, kPlanPer (t +
// 1)) sequentially, so the block does one wave scan per prefix sum.  The
// three prefix sums (pairs, work items, streamed rows) are wave scans, then
// one combine over the wave totals and, with more than one workgroup, the
// totals of the workgroups before (bsum, written by the SUMS pass of the same
// kernel).
constexpr int kPlanPer = 4;
constexpr int kPlanBlk = kPlanPer * kPlanThreads;

__device__ __forceinline__ int64_t wave_incl_scan(int64_t v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

template <bool SUMS>
__global__ __launch_bounds__(kPlanThreads) void k_plan_lists_blk(IvfParams p) {
    constexpr int NWV = kPlanThreads / 64;
    __shared__ int s_cnt[kPlanBlk], s_len[kPlanBlk];
    __shared__ int64_t sh[3][NWV];
    const int base = blockIdx.x * kPlanBlk;
    const int L = min(p.nlist - base, kPlanBlk);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int qs = p.qg == 64 ? 6 : p.qg == 32 ? 5 : 4;  // qg is 16, 32 or 64
    for (int i = t; i < kPlanBlk; i += kPlanThreads) {
        const bool in = i < L;
        s_cnt[i] = in ? p.lcount[base + i] : 0;
        s_len[i] = in ? (int)(p.list_off[base + i + 1] - p.list_off[base + i]) : 0;
    }
    __syncthreads();
    int64_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
    for (int r = 0; r < kPlanPer; ++r) {
        const int c = s_cnt[kPlanPer * t + r], l = s_len[kPlanPer * t + r];
        const int64_t g = (c + p.qg - 1) >> qs;
        a0 += c;
        a1 += g * ((l + p.chunk - 1) / p.chunk);
        a2 += g * l;
    }
    const int64_t i0 = wave_incl_scan(a0), i1 = wave_incl_scan(a1), i2 = wave_incl_scan(a2);
    if (lane == 63) {
        sh[0][wv] = i0;
        sh[1][wv] = i1;
        sh[2][wv] = i2;
    }
    __syncthreads();
    if (SUMS) {
        if (t < 3) {
            int64_t v = 0;
            for (int w = 0; w < NWV; ++w) v += sh[t][w];
            p.bsum[3 * blockIdx.x + t] = v;
        }
        return;
    }
    int64_t c0 = i0 - a0, c1 = i1 - a1, t1 = 0, t2 = 0;
    for (int w = 0; w < NWV; ++w) {
        if (w < wv) {
            c0 += sh[0][w];
            c1 += sh[1][w];
        }
        t1 += sh[1][w];
        t2 += sh[2][w];
    }
    if (gridDim.x > 1) {
        t1 = t2 = 0;
        for (int b = 0; b < (int)gridDim.x; ++b) {
            if (b < (int)blockIdx.x) {
                c0 += p.bsum[3 * b];
                c1 += p.bsum[3 * b + 1];
            }
            t1 += p.bsum[3 * b + 1];
            t2 += p.bsum[3 * b + 2];
        }
    }
#pragma unroll
    for (int r = 0; r < kPlanPer; ++r) {
        const int li = kPlanPer * t + r;
        if (li >= L) break;
        const int c = s_cnt[li], l = s_len[li];
        const int g = (c + p.qg - 1) >> qs;
        const int nc = (l + p.chunk - 1) / p.chunk;
        p.lstart[base + li] = c0;
        p.lfill[base + li] = 0;  // the scatter's cursors (no memset of their own)
        for (int j = 0; j < g; ++j)
            for (int cc = 0; cc < nc; ++cc) {
                p.item_list[c1] = base + li;
                p.item_grp[c1] = j;
                p.item_chk[c1] = cc;
                ++c1;
            }
        c0 += c;
    }
    if (t == 0 && blockIdx.x == 0) {
        *p.nitems = (int)t1;
        p.stats[1] = t1;
        p.stats[2] = t2 * p.dpad * p.esize;
        p.stats[3] = (int64_t)p.nq * p.nprobe;
    }
}

__global__ __launch_bounds__(256) void k_plan_scatter(IvfParams p) {
    const int64_t E = (int64_t)p.nq * p.nprobe;
    const int64_t gt = blockIdx.x * 256ll + threadIdx.x, gs = (int64_t)gridDim.x * 256;
    // pairs grouped by list (order inside a list is free: every pair owns
    // its output region, so results do not depend on it)
    for (int64_t e = gt; e < E; e += gs) {
        const int64_t l = p.probes[e];
        if (l >= 0 && l < p.nlist) {
            const int slot = atomicAdd(&p.lfill[l], 1);
            p.lq[p.lstart[l] + slot] = (int)e;
        }
    }
    // per query: its probes' regions back to back in probe order (offsets
    // relative to the query's region; qstart added by the scan)
    for (int64_t q = gt; q < p.nq; q += gs) {
        int64_t tot = 0;
        for (int r = 0; r < p.nprobe; ++r) {
            const int64_t e = q * p.nprobe + r;
            const int64_t l = p.probes[e];
            p.qbase[e] = tot;
            if (l >= 0 && l < p.nlist) tot += p.list_off[l + 1] - p.list_off[l];
        }
        p.qstart[q] = tot;
    }
}

__global__ __launch_bounds__(kPlanThreads) void k_plan_queries(IvfParams p) {
    __shared__ int64_t sh[kPlanThreads + 1];
    const int64_t total = block_exclusive_scan(
        p.nq, [&](int64_t i) { return p.qstart[i]; }, [&](int64_t i, int64_t v) { p.qstart[i] = v; }, sh);
    if (threadIdx.x == 0) {
        p.qstart[p.nq] = total;
        p.stats[0] = total;  // approximate values written
    }
}

// Plan for few pairs (E = nq * nprobe <= kPlanSmallE; nprobe 1..4 at nq
// 1000), in ONE workgroup: the (list, pair) keys are sorted in LDS, so the
// lists a query batch actually probes are runs of the sorted keys -- the
// general plan above scans every list of the index (39063: zero-fill, count,
// two passes over the lists, scatter, query scan = six launches, ~43 us at
// nq 1000, nprobe 1).  Outputs are the general plan's: lstart / lcount of the
// probed lists (the scan reads no other), the pairs grouped by list in lq,
// items in list order, the query regions (qbase, qstart) and the stats.
constexpr int kPlanSmallE = 4096;
__global__ __launch_bounds__(kPlanThreads) void k_plan_small(IvfParams p) {
    __shared__ uint64_t key[kPlanSmallE];
    __shared__ int64_t sh[kPlanThreads + 1];
    __shared__ unsigned long long s_rows;
    const int t = threadIdx.x;
    const int E = p.nq * p.nprobe;
    const int qs = p.qg == 64 ? 6 : p.qg == 32 ? 5 : 4;  // qg is 16, 32 or 64
    int N = 1;
    while (N < E) N <<= 1;
    for (int i = t; i < N; i += kPlanThreads) {
        uint64_t k = ~0ull;
        if (i < E) {
            const int64_t l = p.probes[i];
            if (l >= 0 && l < p.nlist) k = ((uint64_t)l << 32) | (uint32_t)i;
        }
        key[i] = k;
    }
    if (t == 0) s_rows = 0;
    __syncthreads();
    for (int size = 2; size <= N; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < (N >> 1); i += kPlanThreads) {
                const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = key[lo], b = key[hi];
                if ((b < a) == up) {
                    key[lo] = b;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    // valid keys [0, Ev); a run of one list starts where the list changes
    auto list_at = [&](int i) { return (int)(key[i] >> 32); };
    auto valid = [&](int i) { return key[i] != ~0ull; };
    auto head = [&](int i) { return valid(i) && (i == 0 || list_at(i - 1) != list_at(i)); };
    // run length: the first position of a larger list (binary search)
    auto run_len = [&](int i) {
        const uint64_t bound = ((uint64_t)(uint32_t)list_at(i) + 1) << 32;
        int lo = i + 1, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key[mid] < bound) lo = mid + 1;
            else hi = mid;
        }
        return lo - i;
    };
    auto list_len = [&](int l) { return (int)(p.list_off[l + 1] - p.list_off[l]); };
    const int64_t nitems = block_exclusive_scan(
        N,
        [&](int64_t i) -> int64_t {
            if (!head((int)i)) return 0;
            const int g = (run_len((int)i) + p.qg - 1) >> qs;
            return (int64_t)g * ((list_len(list_at((int)i)) + p.chunk - 1) / p.chunk);
        },
        [&](int64_t i, int64_t r1) {
            if (!valid((int)i)) return;
            const int l = list_at((int)i);
            p.lq[i] = (int)(uint32_t)key[i];
            if (!head((int)i)) return;
            const int c = run_len((int)i), len = list_len(l);
            const int g = (c + p.qg - 1) >> qs, nc = (len + p.chunk - 1) / p.chunk;
            p.lstart[l] = i;
            p.lcount[l] = c;
            atomicAdd(&s_rows, (unsigned long long)g * (unsigned long long)len);
            for (int j = 0; j < g; ++j)
                for (int cc = 0; cc < nc; ++cc) {
                    p.item_list[r1] = l;
                    p.item_grp[r1] = j;
                    p.item_chk[r1] = cc;
                    ++r1;
                }
        },
        sh);
    // per query: its probes' regions back to back in probe order, then the
    // exclusive scan of the query totals
    for (int q = t; q < p.nq; q += kPlanThreads) {
        int64_t tot = 0;
        for (int r = 0; r < p.nprobe; ++r) {
            const int64_t e = (int64_t)q * p.nprobe + r;
            const int64_t l = p.probes[e];
            p.qbase[e] = tot;
            if (l >= 0 && l < p.nlist) tot += p.list_off[l + 1] - p.list_off[l];
        }
        p.qstart[q] = tot;
    }
    __syncthreads();
    const int64_t total = block_exclusive_scan(
        p.nq, [&](int64_t i) { return p.qstart[i]; }, [&](int64_t i, int64_t v) { p.qstart[i] = v; }, sh);
    if (t == 0) {
        p.qstart[p.nq] = total;
        *p.nitems = (int)nitems;
        p.stats[0] = total;
        p.stats[1] = nitems;
        p.stats[2] = (int64_t)s_rows * p.dpad * p.esize;
        p.stats[3] = E;
    }
}

// Plan for the dense case (every query probes every list, probe r = list r:
// the coarse quantizer's centroid chunks), in one grid kernel.
__global__ __launch_bounds__(256) void k_plan_dense(IvfParams p, int64_t npos) {
    const int L = p.nlist, G = (p.nq + p.qg - 1) / p.qg;
    const int64_t E = (int64_t)p.nq * L;
    const int64_t gt = blockIdx.x * 256ll + threadIdx.x, gs = (int64_t)gridDim.x * 256;
    for (int64_t e = gt; e < E; e += gs) {
        const int64_t q = e / L, l = e - q * L;
        p.lq[l * p.nq + q] = (int)e;
        p.qbase[e] = p.list_off[l];
    }
    // items (list, group, slice): lists here are centroid chunks of equal
    // length, so every list has the same slices
    const int NC = (int)((p.list_off[1] - p.list_off[0] + p.chunk - 1) / p.chunk);
    for (int64_t i = gt; i < (int64_t)L * G * NC; i += gs) {
        p.item_list[i] = (int)(i / ((int64_t)G * NC));
        p.item_grp[i] = (int)((i / NC) % G);
        p.item_chk[i] = (int)(i % NC);
    }
    for (int64_t l = gt; l < L; l += gs) {
        p.lcount[l] = p.nq;
        p.lstart[l] = l * p.nq;
    }
    for (int64_t q = gt; q <= p.nq; q += gs) p.qstart[q] = q * npos;
    if (gt == 0) {
        *p.nitems = L * G * NC;
        p.stats[0] = (int64_t)p.nq * npos;
        p.stats[1] = (int64_t)L * G * NC;
        p.stats[2] = (int64_t)G * npos * p.dpad * p.esize;
        p.stats[3] = E;
    }
}

// probes[q][j] = j: every query probes every list (the coarse quantizer's
// centroid chunks)
__global__ __launch_bounds__(256) void k_iota_probes(int64_t *probes, int64_t E, int np) {
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) probes[e] = e % np;
}

// ---- launchers -------------------------------------------------------------

void launch_ivf_plan_dense(const IvfParams &p, int64_t npos, hipStream_t s) {
    const int64_t E = (int64_t)p.nq * p.nlist;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((E + 255) / 256, 2048));
    hipLaunchKernelGGL(k_plan_dense, dim3(grid), dim3(256), 0, s, p, npos);
}

void launch_iota_probes(int64_t *probes, int nq, int np, hipStream_t s) {
    const int64_t E = (int64_t)nq * np;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((E + 255) / 256, 1024));
    hipLaunchKernelGGL(k_iota_probes, dim3(grid), dim3(256), 0, s, probes, E, np);
}

void launch_ivf_plan(const IvfParams &p, hipStream_t s) {
    const int64_t E = (int64_t)p.nq * p.nprobe;
    if (E <= kPlanSmallE) {
        hipLaunchKernelGGL(k_plan_small, dim3(1), dim3(kPlanThreads), 0, s, p);
        return;
    }
    // (lfill: zeroed by the list pass; a fill kernel, not hipMemsetAsync: the
    // runtime's fill took two launches)
    launch_fill2(reinterpret_cast<uint32_t *>(p.lcount), p.nlist, 0u, nullptr, 0, 0u, s);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((std::max(E, (int64_t)p.nq) + 255) / 256, 2048));
    hipLaunchKernelGGL(k_plan_count, dim3(grid), dim3(256), 0, s, p);
    const int nb = (p.nlist + kPlanBlk - 1) / kPlanBlk;
    if (nb > 1) hipLaunchKernelGGL(k_plan_lists_blk<true>, dim3(nb), dim3(kPlanThreads), 0, s, p);
    hipLaunchKernelGGL(k_plan_lists_blk<false>, dim3(std::max(nb, 1)), dim3(kPlanThreads), 0, s, p);
    hipLaunchKernelGGL(k_plan_scatter, dim3(grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_plan_queries, dim3(1), dim3(kPlanThreads), 0, s, p);
}

}  // namespace mqvs
