// kernels_segprep.hip -- segment preparation: row norms, the cosine
// normalisation of the rows, the synthetic generator and the nonempty pack.
#include "flat_kernels.h"

namespace mqvs {

constexpr int NB_K = 32;
constexpr int NB_LD = NB_K + 4;

// Per-row squared norm, sequential fp32 with the product rounded then added
// (VectorDataset.h:105-108 for normalize; fvec_norm_L2sqr for the BLAS branch
// norms, the same order the KATs pin for fvec_*).  Rows staged through LDS so
// the HBM reads stay coalesced while each lane walks its own row in order.
__device__ void block_row_sumsq(const float *rows, int64_t r0, int64_t r1, int d,
                                float (*tile)[256 * NB_LD], float &sum) {
    const int t = threadIdx.x;
    sum = 0.0f;
    const int nst = (d + NB_K - 1) / NB_K;
    for (int s = 0; s < nst; ++s) {
        const int k0 = s * NB_K;
        for (int i = 0; i < 8; ++i) {
            const int f = t + 256 * i;
            const int lr = f >> 3, c = (f & 7) * 4;
            const int64_t gr = r0 + lr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr < r1) {
                const float *src = rows + gr * d + k0 + c;
                if (k0 + c + 0 < d) v.x = src[0];
                if (k0 + c + 1 < d) v.y = src[1];
                if (k0 + c + 2 < d) v.z = src[2];
                if (k0 + c + 3 < d) v.w = src[3];
            }
            *reinterpret_cast<float4 *>(&tile[0][lr * NB_LD + c]) = v;
        }
        __syncthreads();
        const float *tl = &tile[0][t * NB_LD];
        const int lim = (d - k0) < NB_K ? (d - k0) : NB_K;
        for (int kk = 0; kk < lim; ++kk) sum = sum + tl[kk] * tl[kk];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_row_norms(const float *rows, int64_t n, int d,
                                                    float *norms) {
    __shared__ __attribute__((aligned(16))) float tile[1][256 * NB_LD];
    for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < n; r0 += (int64_t)gridDim.x * 256) {
        const int64_t r1 = r0 + 256 < n ? r0 + 256 : n;
        float sum;
        block_row_sumsq(rows, r0, r1, d, tile, sum);
        if (r0 + threadIdx.x < r1) norms[r0 + threadIdx.x] = sum;
    }
}

// VectorDataset<Float>::normalize (VectorDataset.h:98-117), in place.
__global__ __launch_bounds__(256) void k_normalize_rows(float *rows, int64_t n, int d) {
    __shared__ __attribute__((aligned(16))) float tile[1][256 * NB_LD];
    __shared__ float scale[256];
    const float eps = 1.1920929e-07f;  // FLT_EPSILON
    for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < n; r0 += (int64_t)gridDim.x * 256) {
        const int64_t r1 = r0 + 256 < n ? r0 + 256 : n;
        float sum;
        block_row_sumsq(rows, r0, r1, d, tile, sum);
        // 0 marks "skip" (sum < FLT_EPSILON): the row is left untouched
        scale[threadIdx.x] = (sum < eps) ? 0.0f : sqrtf(sum);
        __syncthreads();
        const int64_t cnt = (r1 - r0) * d;
        float *base = rows + r0 * d;
        for (int64_t i = threadIdx.x; i < cnt; i += 256) {
            const float s = scale[i / d];
            if (s != 0.0f) base[i] = base[i] / s;
        }
        __syncthreads();
    }
}

void launch_row_norms(const float *rows, int64_t n, int d, float *norms, hipStream_t s) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) return;
    hipLaunchKernelGGL(k_row_norms, dim3((unsigned)blocks), dim3(256), 0, s, rows, n, d, norms);
}

void launch_normalize_rows(float *rows, int64_t n, int d, hipStream_t s) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) return;
    hipLaunchKernelGGL(k_normalize_rows, dim3((unsigned)blocks), dim3(256), 0, s, rows, n, d);
}

// Counter-based synthetic generator; bit-identical to oracle/mqvs_oracle.c
// orc_generate (integer hash, exact 16-bit fractions, one rounding).
__device__ __host__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

__device__ inline float gen_gauss(uint64_t seed, uint64_t idx) {
    const uint64_t h = splitmix64(seed ^ idx);
    const float u0 = (float)(h & 0xffff) * (1.0f / 65536.0f);
    const float u1 = (float)((h >> 16) & 0xffff) * (1.0f / 65536.0f);
    const float u2 = (float)((h >> 32) & 0xffff) * (1.0f / 65536.0f);
    const float u3 = (float)((h >> 48) & 0xffff) * (1.0f / 65536.0f);
    const float s = (u0 + u1) + (u2 + u3);
    return (s - 2.0f) * 1.7320508f;
}

__global__ void k_generate(uint64_t seed, int mode, int64_t row0, int64_t n, int d, float *out) {
    const int64_t total = n * d;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / d;
        const int j = (int)(e - r * d);
        const uint64_t row = (uint64_t)(row0 + r);
        const uint64_t idx = row * (uint64_t)d + (uint64_t)j;
        float v;
        if (mode == 0) {
            v = (float)((int)(splitmix64(seed ^ idx) % 17ULL) - 8);
        } else if (mode == 1) {
            v = gen_gauss(seed, idx);
        } else if (mode == 2) {
            const uint64_t c =
                splitmix64(seed ^ 0xC0FFEEULL ^ (row * 0x100000001B3ULL)) % 4096ULL;
            const float center = gen_gauss(seed ^ 0xCE17E5ULL, c * (uint64_t)d + (uint64_t)j);
            v = center + 0.25f * gen_gauss(seed, idx);
        } else {
            // hard mixture: 65536 centres, noise as large as the centres
            const uint64_t c =
                splitmix64(seed ^ 0xC0FFEEULL ^ (row * 0x100000001B3ULL)) % 65536ULL;
            const float center = gen_gauss(seed ^ 0xCE17E5ULL, c * (uint64_t)d + (uint64_t)j);
            v = center + gen_gauss(seed, idx);
        }
        out[e] = v;
    }
}

void launch_generate(uint64_t seed, int mode, int64_t row0, int64_t n, int d, float *out,
                     hipStream_t s) {
    const int64_t total = n * d;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (blocks < 1) return;
    hipLaunchKernelGGL(k_generate, dim3((unsigned)blocks), dim3(256), 0, s, seed, mode, row0, n, d,
                       out);
}

// bytes (1 = nonempty) -> LSB-first bitmap
__global__ void k_pack(const uint8_t *bytes, int64_t n, uint8_t *bits) {
    const int64_t nb = (n + 7) / 8;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb;
         b += (int64_t)gridDim.x * blockDim.x) {
        uint8_t v = 0;
        for (int i = 0; i < 8; ++i) {
            const int64_t r = b * 8 + i;
            if (r < n && bytes[r]) v |= (uint8_t)(1u << i);
        }
        bits[b] = v;
    }
}

void launch_pack_nonempty(const uint8_t *bytes, int64_t n, uint8_t *bits, hipStream_t s) {
    int64_t blocks = ((n + 7) / 8 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (blocks < 1) return;
    hipLaunchKernelGGL(k_pack, dim3((unsigned)blocks), dim3(256), 0, s, bytes, n, bits);
}

}  // namespace mqvs
