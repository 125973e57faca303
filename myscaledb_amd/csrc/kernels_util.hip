// kernels_util.hip -- one-kernel utilities of the host paths (fills, words to
// pinned host memory, the ASYNC flags, the id map of decoupled parts) and the
// benchmark's HBM read sweep.
#include "flat_kernels.h"

namespace mqvs {

// Up to two 32-bit fills in one launch (the small status / counter / list-tail
// fills of a search: a runtime memset is a ~4 us kernel of its own each)
__global__ void k_fill2(uint32_t *a, int64_t na, uint32_t va, uint32_t *b, int64_t nb, uint32_t vb) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += stride) {
        if (i < na)
            a[i] = va;
        else
            b[i - na] = vb;
    }
}

void launch_fill2(uint32_t *a, int64_t na, uint32_t va, uint32_t *b, int64_t nb, uint32_t vb, hipStream_t s) {
    if (!a) na = 0;
    if (!b) nb = 0;
    const int64_t n = na + nb;
    if (n <= 0) return;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_fill2, dim3((unsigned)blocks), dim3(256), 0, s, a, na, va, b, nb, vb);
}

__global__ __launch_bounds__(256) void k_words_to_host(const int64_t *a, int na, const int *b, int nb, int64_t *ha,
                                                      int *hb, const int64_t *pq, int npq) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (pq) {
        // column sums of pq[npq][na] (na <= 4): each thread its rows' na
        // words (independent loads, 4 rows in flight), then the block sum
        __shared__ int64_t part[4][4];
        int64_t v[4] = {0, 0, 0, 0};
#pragma unroll 4
        for (int r = t; r < npq; r += 256)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < na) v[c] += pq[(int64_t)r * na + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off);
            if (lane == 0) part[wv][c] = v[c];
        }
        __syncthreads();
        if (t < na) *reinterpret_cast<volatile int64_t *>(ha + t) = part[0][t] + part[1][t] + part[2][t] + part[3][t];
    } else if (t < na) {
        *reinterpret_cast<volatile int64_t *>(ha + t) = a[t];
    }
    if (t < nb) *reinterpret_cast<volatile int *>(hb + t) = b[t];
    __threadfence_system();
}

void launch_words_to_host(const int64_t *a, int na, const int *b, int nb, int64_t *host_a, int *host_b,
                          hipStream_t s, const int64_t *pq, int npq) {
    if (pq && na > 4) fail(MQVS_ERR_LOGICAL, "words_to_host: more than 4 summed columns");
    hipLaunchKernelGGL(k_words_to_host, dim3(1), dim3(pq ? 256 : 64), 0, s, a, na, b, nb, host_a, host_b, pq, npq);
}

// ---------------------------------------------------------------------------
// ASYNC outcome of a search, OR-ed into the thread's sticky word
// (mqvs_async_check)
__global__ void k_async_flags(const int *overflow, const int *status, int status_matters, int *sticky) {
    if (threadIdx.x != 0) return;
    int w = 0;
    if (overflow && overflow[0]) w |= 1;
    if (status && status_matters && status[0]) w |= 2;
    if (w) atomicOr(sticky, w);
}

void launch_async_flags(const int *overflow, const int *status, int status_matters, int *sticky, hipStream_t s) {
    hipLaunchKernelGGL(k_async_flags, dim3(1), dim3(64), 0, s, overflow, status, status_matters, sticky);
}

// ---------------------------------------------------------------------------
// Decoupled parts (a merged part whose vector index still lives in its source
// parts): VIWithColumnInPart::transferToNewRowIds (VIWithDataPart.cpp:56-67)
// on the device (the filter map, getRealBitmap, is in kernels_filter.hip).
__global__ void k_map_ids(int64_t *ids, int64_t count, const uint64_t *map) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = ids[i];
        if (v >= 0) ids[i] = (int64_t)map[v];
    }
}

void launch_map_ids(int64_t *ids, int64_t count, const uint64_t *map, hipStream_t s) {
    if (count <= 0) return;
    const int64_t blocks = std::min<int64_t>((count + 255) / 256, 4096);
    hipLaunchKernelGGL(k_map_ids, dim3((unsigned)blocks), dim3(256), 0, s, ids, count, map);
}

// ---------------------------------------------------------------------------
// STREAM-like HBM read sweep (bench utility: the measured denominator of the
// scan's HBM fraction).  Every lane reads 16 B per load, 4 loads in flight per
// lane per iteration, grid-stride over the whole buffer; the XOR of what it
// read keeps the loads live (written only when it equals an impossible
// pattern).
typedef unsigned rs_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_read_sweep(const rs_u32x4 *p, int64_t n16, unsigned *sink) {
    rs_u32x4 acc = {0u, 0u, 0u, 0u};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const rs_u32x4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
        acc ^= a ^ b ^ c ^ d;
    }
    for (; i < n16; i += stride) acc ^= p[i];
    if (acc.x == 0x9E3779B9u && acc.y == 0x7F4A7C15u && acc.z == acc.w) sink[0] = acc.x;
}

// The same bytes, each workgroup over one contiguous slice: per round its 256
// lanes read U consecutive 4 KiB pieces (U loads in flight per lane,
// non-temporal: every byte is read once), so DRAM pages are swept in order.
template <int U>
__global__ __launch_bounds__(256) void k_read_slices(const rs_u32x4 *p, int64_t n16, unsigned *sink) {
    rs_u32x4 acc = {0u, 0u, 0u, 0u};
    const int64_t per = (n16 + gridDim.x - 1) / gridDim.x;
    const int64_t b = (int64_t)blockIdx.x * per, e = b + per < n16 ? b + per : n16;
    int64_t i = b + threadIdx.x;
    for (; i + (U - 1) * 256 < e; i += U * 256) {
        rs_u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(p + i + u * 256);
#pragma unroll
        for (int u = 0; u < U; ++u) acc ^= v[u];
    }
    for (; i < e; i += 256) acc ^= p[i];
    if (acc.x == 0x9E3779B9u && acc.y == 0x7F4A7C15u && acc.z == acc.w) sink[0] = acc.x;
}

// best time of `reps` sweeps over a fresh `bytes` buffer (filled first, so
// the sweep reads written pages) on stream s, over the sweep shapes (the
// grid-stride k_read_sweep at 8 workgroups per CU; contiguous slices at 4 and
// 8 workgroups per CU with 8 or 16 loads in flight): the best is the
// achievable read rate the bench reports beside the plane scans
double measure_read_sweep(size_t bytes, int reps, hipStream_t s, double *best_ms) {
    const int cus = device_cus();
    bytes = bytes / 16 * 16;
    void *buf = nullptr;
    MQVS_HIP(hipMalloc(&buf, bytes + 256));
    unsigned *sink = reinterpret_cast<unsigned *>(static_cast<char *>(buf) + bytes);
    MQVS_HIP(hipMemsetAsync(buf, 0x5A, bytes, s));
    hipEvent_t e0, e1;
    MQVS_HIP(hipEventCreate(&e0));
    MQVS_HIP(hipEventCreate(&e1));
    const int64_t n16 = (int64_t)(bytes / 16);
    const auto *src = static_cast<const rs_u32x4 *>(buf);
    float best = 1e30f;
    for (int shape = 0; shape < 5; ++shape) {
        for (int r = 0; r <= reps; ++r) {  // (pass 0 warms up)
            MQVS_HIP(hipEventRecord(e0, s));
            switch (shape) {
                case 0: hipLaunchKernelGGL(k_read_sweep, dim3(cus * 8), dim3(256), 0, s, src, n16, sink); break;
                case 1: hipLaunchKernelGGL(k_read_slices<8>, dim3(cus * 4), dim3(256), 0, s, src, n16, sink); break;
                case 2: hipLaunchKernelGGL(k_read_slices<8>, dim3(cus * 8), dim3(256), 0, s, src, n16, sink); break;
                case 3: hipLaunchKernelGGL(k_read_slices<16>, dim3(cus * 4), dim3(256), 0, s, src, n16, sink); break;
                default: hipLaunchKernelGGL(k_read_slices<16>, dim3(cus * 2), dim3(256), 0, s, src, n16, sink); break;
            }
            MQVS_HIP(hipEventRecord(e1, s));
            MQVS_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            MQVS_HIP(hipEventElapsedTime(&ms, e0, e1));
            if (r > 0 && ms < best) best = ms;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    if (best_ms) *best_ms = best;
    return (double)bytes / (best * 1e-3) / 1e9;
}

}  // namespace mqvs
