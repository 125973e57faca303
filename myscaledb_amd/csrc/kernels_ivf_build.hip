// kernels_ivf_build.hip -- what an index build launches (index_build.hip;
// index_kernels.h has the layout): the list planes, the k-means helpers and
// the grouping of the rows by list.
#include "index_kernels.h"

namespace mqvs {

// ---- build kernels ---------------------------------------------------------

// plane[pos] = bf16(rows[perm[pos]]) (zero for padding and columns >= d),
// pnorm[pos] = |y|^2
__global__ __launch_bounds__(256) void k_ivf_pack(const float *rows, const float *norms, int d,
                                                  const int32_t *perm, int64_t npos, int64_t dpad,
                                                  uint16_t *plane, float *pnorm) {
    const int64_t c8 = dpad / 8;
    const int64_t total = npos * c8;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pos = i / c8, cc = i - pos * c8;
        const int32_t row = perm[pos];
        uint16_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t col = cc * 8 + j;
            const float x = (row >= 0 && col < d) ? rows[(int64_t)row * d + col] : 0.f;
            v[j] = f32_to_bf16_rn(x);
        }
        uint4 o;
        o.x = v[0] | ((uint32_t)v[1] << 16);
        o.y = v[2] | ((uint32_t)v[3] << 16);
        o.z = v[4] | ((uint32_t)v[5] << 16);
        o.w = v[6] | ((uint32_t)v[7] << 16);
        // 16-position blocks of 32-column pieces (1 KiB each): see k_ivf_scan
        const int64_t col0 = cc * 8;
        *reinterpret_cast<uint4 *>(plane + ((pos >> 4) * (dpad / 32) + (col0 >> 5)) * 512 + (pos & 15) * 32 +
                                   (col0 & 31)) = o;
        if (cc == 0) pnorm[pos] = row >= 0 ? norms[row] : 0.f;
    }
}

// ---- fp8 list plane (plane=fp8) --------------------------------------------

// the value of an e4m3fn code (exact)
__device__ inline float e4m3_value(uint32_t c) {
    const uint32_t e = (c >> 3) & 15u, m = c & 7u;
    float v;
    if (e == 15u && m == 7u)
        v = __builtin_nanf("");
    else if (e == 0u)
        v = (float)m * 0x1p-9f;
    else
        v = __builtin_bit_cast(float, ((e + 120u) << 23) | (m << 20));  // 2^(e - 7) (1 + m / 8)
    return (c & 0x80u) ? -v : v;
}

// The quantiser of include/mqvs.h (mqvs_index_build, plane=fp8), one wave per
// vector: amax and its frexp exponent E, scale exponent e = 8 - E (0 for a zero
// or non-finite amax), codes = e4m3fn(x_i 2^e) by the hardware conversion
// (round to nearest even; scaled magnitudes of a finite vector lie under 256;
// a scaled value that is not within 448 -- a vector with a non-finite element
// only -- is stored as the NaN code).  Norm records as k_to_hi's, with v8 =
// the de-scaled codes: [0] |v8|, [1] |v - v8|, [6] |v|, summed in fp64 (the
// first two in the scaled domain, where codes and residuals are exact) and
// rounded up; their maxima over the vectors that are not padding (maxrec) are
// the list plane's record for k_query_bound.  A non-finite element makes the
// sums, and so the maxima, non-finite (NaN counts as +inf), which turns the
// re-rank's bound pruning off.
//
// Output: codes (the list plane, blocked [m / 16][dpad / 64][16][64] bytes), or
// hi (queries: the scaled codes' values as bf16, which holds every e4m3 value,
// row-major [m][dpad]: the B operand of k_ivf_scan_fp8).
__global__ __launch_bounds__(256) void k_to_fp8(const float *src, int64_t sld, int d, const int32_t *perm, int64_t m,
                                                int64_t dpad, uint8_t *codes, uint16_t *hi, int16_t *expo,
                                                const float *norms, float *pnorm, float *rec, float *maxrec) {
    __shared__ unsigned smax[4][3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned mx[3] = {0u, 0u, 0u};  // running maxima (bit patterns of non-negative floats; NaN -> +inf)
    for (int64_t v = (int64_t)blockIdx.x * 4 + w; v < m; v += (int64_t)gridDim.x * 4) {
        const int64_t row = perm ? (int64_t)perm[v] : v;
        const float *x = row >= 0 ? src + row * sld : nullptr;
        float amax = 0.f;
        if (x)
            for (int i = lane; i < d; i += 64) {
                const float a = fabsf(x[i]);
                amax = fmaxf(amax, a == a ? a : __builtin_inff());
            }
        for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
        int e = 0;
        if (amax > 0.f && amax < __builtin_inff()) {
            // amax = f 2^E, f in [0.5, 1) (subnormals included)
            const uint32_t bits = __builtin_bit_cast(uint32_t, amax), ex = bits >> 23;
            const int E = ex ? (int)ex - 126 : -149 + (32 - __clz((int)(bits & 0x7FFFFFu)));
            e = 8 - E;
        }
        uint8_t *out = codes ? codes + (v >> 4) * 16 * dpad + (v & 15) * 64 : nullptr;
        double nx = 0, nh = 0, nr = 0;
        for (int64_t i = 4 * lane; i < dpad; i += 256) {
            float xv[4], sv[4];
            bool in[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xv[j] = (x && i + j < d) ? x[i + j] : 0.f;
                sv[j] = ldexpf(xv[j], e);
                in[j] = fabsf(sv[j]) <= 448.f;
            }
            int pk = __builtin_amdgcn_cvt_pk_fp8_f32(in[0] ? sv[0] : 0.f, in[1] ? sv[1] : 0.f, 0, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(in[2] ? sv[2] : 0.f, in[3] ? sv[3] : 0.f, pk, true);
            uint32_t word = 0;
            uint16_t hb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t code = ((uint32_t)pk >> (8 * j)) & 0xFFu;
                if (!in[j]) code = 0x7Fu | ((__builtin_bit_cast(uint32_t, sv[j]) >> 24) & 0x80u);
                word |= code << (8 * j);
                const float hf = e4m3_value(code);
                hb[j] = (uint16_t)(__builtin_bit_cast(uint32_t, hf) >> 16);  // exact: 4 significant bits
                const double hv = (double)hf, rv = (double)sv[j] - hv;
                nx += (double)xv[j] * xv[j];
                nh += hv * hv;
                nr += rv * rv;
            }
            if (out) *reinterpret_cast<uint32_t *>(out + (i >> 6) * 1024 + (i & 63)) = word;
            if (hi)
                *reinterpret_cast<uint2 *>(hi + v * dpad + i) =
                    make_uint2(hb[0] | ((uint32_t)hb[1] << 16), hb[2] | ((uint32_t)hb[3] << 16));
        }
        for (int off = 32; off > 0; off >>= 1) {
            nx += __shfl_xor(nx, off);
            nh += __shfl_xor(nh, off);
            nr += __shfl_xor(nr, off);
        }
        if (lane == 0) {
            expo[v] = (int16_t)e;
            if (pnorm) pnorm[v] = row >= 0 ? norms[row] : 0.f;
        }
        if (row < 0) continue;  // padding: no record
        // (scaled sums back to the vector's units; rounded up)
        const float r[kMxRec] = {(float)(ldexp(sqrt(nh), -e) * (1.0 + 1e-7)),
                                 (float)(ldexp(sqrt(nr), -e) * (1.0 + 1e-7)),
                                 0.f, 0.f, 0.f, 0.f,
                                 (float)(sqrt(nx) * (1.0 + 1e-7)), 0.f};
        if (rec && lane < kMxRec) {
            float rv = 0.f;
#pragma unroll
            for (int t = 0; t < kMxRec; ++t)
                if (lane == t) rv = r[t];
            rec[v * kMxRec + lane] = rv;
        }
        const int slot[3] = {0, 1, 6};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const float f = r[slot[t]];
            const unsigned b = (f == f) ? __builtin_bit_cast(unsigned, f) : 0x7F800000u;
            mx[t] = b > mx[t] ? b : mx[t];
        }
    }
    if (!maxrec) return;
    if (lane == 0)
        for (int t = 0; t < 3; ++t) smax[w][t] = mx[t];
    __syncthreads();
    if (threadIdx.x < 3) {
        const int t = threadIdx.x;
        unsigned b = smax[0][t];
        for (int ww = 1; ww < 4; ++ww) b = smax[ww][t] > b ? smax[ww][t] : b;
        atomicMax(reinterpret_cast<unsigned *>(maxrec) + (t == 2 ? 6 : t), b);
    }
}

// dst[i] = src[idx[i]] (rows of d floats, source row stride src_ld; idx null = identity)
__global__ __launch_bounds__(256) void k_gather_rows(const float *src, int64_t src_ld, int d, const int64_t *idx,
                                                     int64_t m, float *dst) {
    const int64_t total = m * d;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / d, col = i - r * d;
        dst[i] = src[(idx ? idx[r] : r) * src_ld + col];
    }
}

// k-means update: centroid c = mean of its members (rows order[off[c]..off[c+1]),
// summed in that order, so the result is deterministic); empty clusters keep
// their centroid.
__global__ __launch_bounds__(256) void k_centroid_mean(const float *rows, int d, const int32_t *order,
                                                       const int64_t *off, float *cent) {
    const int c = blockIdx.x;
    const int64_t b = off[c], e = off[c + 1];
    if (e <= b) return;
    const float inv = 1.0f / (float)(e - b);
    for (int j = threadIdx.x; j < d; j += 256) {
        float s = 0.f;
        for (int64_t i = b; i < e; ++i) s += rows[(int64_t)order[i] * d + j];
        cent[(int64_t)c * d + j] = s * inv;
    }
}

// ---- launchers -------------------------------------------------------------

void launch_ivf_pack(const float *rows, const float *norms, int d, const int32_t *perm, int64_t npos, int64_t dpad,
                     uint16_t *plane, float *pnorm, hipStream_t s) {
    const int64_t total = npos * (dpad / 8);
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 65536);
    if (grid > 0) hipLaunchKernelGGL(k_ivf_pack, dim3(grid), dim3(256), 0, s, rows, norms, d, perm, npos, dpad, plane, pnorm);
}

void launch_to_fp8(const float *src, int64_t src_ld, int d, const int32_t *perm, int64_t m, int64_t dpad,
                   uint8_t *codes, uint16_t *hi, int16_t *expo, const float *norms, float *pnorm, float *rec,
                   float *maxrec, hipStream_t s) {
    if (m <= 0) return;
    const int64_t blocks = std::min<int64_t>((m + 3) / 4, (int64_t)device_cus() * 16);
    hipLaunchKernelGGL(k_to_fp8, dim3((unsigned)blocks), dim3(256), 0, s, src, src_ld, d, perm, m, dpad, codes, hi,
                       expo, norms, pnorm, rec, maxrec);
}

void launch_gather_rows(const float *src, int64_t src_ld, int d, const int64_t *idx, int64_t m, float *dst,
                        hipStream_t s) {
    const int64_t total = m * d;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 65536);
    if (grid > 0) hipLaunchKernelGGL(k_gather_rows, dim3(grid), dim3(256), 0, s, src, src_ld, d, idx, m, dst);
}

void launch_centroid_mean(const float *rows, int d, const int32_t *order, const int64_t *off, int nlist, float *cent,
                          hipStream_t s) {
    if (nlist > 0) hipLaunchKernelGGL(k_centroid_mean, dim3(nlist), dim3(256), 0, s, rows, d, order, off, cent);
}

// ---------------------------------------------------------------------------
// Rows grouped by list on the device (index.hip: finish_index, the tail of
// both builds and of mqvs_index_load).  Input: the canonical assignment
// assign[n] (list id, -1 = in no list).  Output: list_off[L + 1] with every
// list's length rounded up to `pad`, and perm[npos]: position list_off[l] + j
// holds the j-th smallest row of list l, every other position -1 -- what a
// stable counting sort of the rows by list id gives.
//   k_grp_count    range check of every value (status word, read by the host
//                  before perm exists) + rows per list
//   k_grp_scan     offsets, npos, longest list, rows in lists (one workgroup)
//   k_grp_scatter  rows to their list's positions through atomic cursors: the
//                  order within a list is whatever the atomics gave
//   k_grp_sort     every run of kSortCap positions of a list sorted ascending
//                  in LDS: lists up to kSortCap rows are then final
//   k_grp_merge    longer lists: sorted runs merged pairwise through a second
//                  buffer, doubling the run length per pass; an element's
//                  place is its index in its run + the elements of the sibling
//                  run below it (rows are distinct)
// The result is a function of assign alone: the atomics only choose which
// order the sort receives.

// the wave's next slots of ctr[a] for its valid lanes: one atomic for the wave
// when they all have the same list (one list holding every row would
// serialise n atomics on one word), else one per lane.  Every lane of the
// wave calls it.
__device__ inline int grp_take(int *ctr, int32_t a, bool valid) {
    const uint64_t m = __ballot(valid);
    if (m == 0) return 0;
    const int lane = threadIdx.x & 63;
    const int first = __ffsll((long long)m) - 1;
    const int32_t a0 = __shfl(a, first);
    if (__ballot(valid && a == a0) == m) {
        int base = 0;
        if (lane == first) base = atomicAdd(&ctr[a0], (int)__popcll(m));
        base = __shfl(base, first);
        return base + (int)__popcll(m & ((1ull << lane) - 1ull));
    }
    return valid ? atomicAdd(&ctr[a], 1) : 0;
}

// (a row whose array is empty is in no list whatever the assignment says)
__global__ __launch_bounds__(256) void k_grp_count(const int32_t *assign, int64_t n, int64_t L,
                                                   const uint8_t *nonempty, int allow_none, int *cnt, int *status) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = blockIdx.x * 256ll + (threadIdx.x & ~63); base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + lane;
        int32_t a = -1;
        if (i < n) {
            a = assign[i];
            if (a < -1 || (int64_t)a >= L) {
                atomicOr(status, kGrpStatusBadRange);
                a = -1;
            } else if (a < 0 && !allow_none) {
                atomicOr(status, kGrpStatusNoList);
            }
            if (nonempty && !bit_test(nonempty, i)) a = -1;
        }
        (void)grp_take(cnt, a, a >= 0);
    }
}

// info: [0] npos, [1] longest list in positions, [2] rows in lists, [3] rows of the longest list, [4] status
__global__ __launch_bounds__(1024) void k_grp_scan(const int *cnt, int64_t L, int pad, int64_t *off, int64_t *info,
                                                   const int *status) {
    __shared__ int64_t s_sum[1024];
    __shared__ unsigned long long s_red[3];
    const int t = threadIdx.x;
    if (t < 3) s_red[t] = 0;
    const int64_t per = (L + 1023) / 1024;
    const int64_t b = min(L, t * per), e = min(L, b + per);
    int64_t sum = 0, mxp = 0, mxc = 0, rows = 0;
    for (int64_t l = b; l < e; ++l) {
        const int64_t c = cnt[l], p = (c + pad - 1) / pad * pad;
        sum += p;
        rows += c;
        mxp = max(mxp, p);
        mxc = max(mxc, c);
    }
    s_sum[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = t >= o ? s_sum[t - o] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    atomicMax(&s_red[0], (unsigned long long)mxp);
    atomicAdd(&s_red[1], (unsigned long long)rows);
    atomicMax(&s_red[2], (unsigned long long)mxc);
    int64_t run = s_sum[t] - sum;
    for (int64_t l = b; l < e; ++l) {
        off[l] = run;
        run += ((int64_t)cnt[l] + pad - 1) / pad * pad;
    }
    __syncthreads();
    if (t == 0) {
        off[L] = s_sum[1023];
        info[0] = s_sum[1023];
        info[1] = (int64_t)s_red[0];
        info[2] = (int64_t)s_red[1];
        info[3] = (int64_t)s_red[2];
        info[4] = *status;
    }
}

__global__ __launch_bounds__(256) void k_grp_scatter(const int32_t *assign, int64_t n, int64_t L,
                                                     const uint8_t *nonempty, const int64_t *off, int *fill,
                                                     int32_t *perm) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = blockIdx.x * 256ll + (threadIdx.x & ~63); base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + lane;
        int32_t a = -1;
        if (i < n) {
            a = assign[i];
            if (a < 0 || (int64_t)a >= L || (nonempty && !bit_test(nonempty, i))) a = -1;
        }
        const int j = grp_take(fill, a, a >= 0);
        if (a >= 0) perm[off[a] + j] = (int32_t)i;
    }
}

// blockIdx.x strides the lists, blockIdx.y a list's runs of kSortCap positions
__global__ __launch_bounds__(256) void k_grp_sort(int32_t *perm, const int64_t *off, const int *cnt, int64_t L) {
    __shared__ int32_t s_row[kSortCap];
    const int t = threadIdx.x;
    for (int64_t l = blockIdx.x; l < L; l += gridDim.x) {
        const int64_t c = cnt[l];
        if (c < 2) continue;
        const int64_t p0 = off[l];
        for (int64_t u0 = (int64_t)blockIdx.y * kSortCap; u0 < c; u0 += (int64_t)gridDim.y * kSortCap) {
            const int len = (int)min((int64_t)kSortCap, c - u0);
            int N = 2;
            while (N < len) N <<= 1;
            for (int i = t; i < N; i += 256) s_row[i] = i < len ? perm[p0 + u0 + i] : 0x7FFFFFFF;
            __syncthreads();
            for (int size = 2; size <= N; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = t; i < (N >> 1); i += 256) {
                        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                        const int32_t x = s_row[lo], y = s_row[hi];
                        if ((x > y) == ((lo & size) == 0)) {
                            s_row[lo] = y;
                            s_row[hi] = x;
                        }
                    }
                    __syncthreads();
                }
            }
            for (int i = t; i < len; i += 256) perm[p0 + u0 + i] = s_row[i];
            __syncthreads();
        }
    }
}

// the list of position pos: the last l with off[l] <= pos (empty lists share
// their successor's offset; pos < off[L])
__device__ inline int64_t grp_list_of_pos(const int64_t *off, int64_t L, int64_t pos) {
    int64_t lo = 0, hi = L - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= pos)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// one merge pass: sorted runs of `width` rows of every list longer than
// kSortCap, src -> dst; every other position is copied
__global__ __launch_bounds__(256) void k_grp_merge(const int32_t *src, int32_t *dst, const int64_t *off,
                                                   const int *cnt, int64_t L, int64_t npos, int64_t width) {
    for (int64_t pos = blockIdx.x * 256ll + threadIdx.x; pos < npos; pos += (int64_t)gridDim.x * 256) {
        const int64_t l = grp_list_of_pos(off, L, pos);
        const int64_t p0 = off[l], j = pos - p0, c = cnt[l];
        const int32_t v = src[pos];
        const int64_t a0 = j / (2 * width) * (2 * width), b0 = a0 + width;
        if (c <= kSortCap || j >= c || b0 >= c) {
            dst[pos] = v;
            continue;
        }
        const bool in_a = j < b0;
        // the sibling run, and how many of its rows are below v
        const int32_t *sib = src + p0 + (in_a ? b0 : a0);
        const int64_t sn = in_a ? min(width, c - b0) : width;
        int64_t lo = 0, hi = sn;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (sib[mid] < v)
                lo = mid + 1;
            else
                hi = mid;
        }
        dst[p0 + a0 + (j - (in_a ? a0 : b0)) + lo] = v;
    }
}

// the canonical assignment of a built index: assign[perm[pos]] = list of pos
// (assign filled with -1 by the caller)
__global__ __launch_bounds__(256) void k_grp_assign_of(const int32_t *perm, const int64_t *off, int64_t L,
                                                       int64_t npos, int64_t n, int32_t *assign) {
    for (int64_t pos = blockIdx.x * 256ll + threadIdx.x; pos < npos; pos += (int64_t)gridDim.x * 256) {
        const int32_t r = perm[pos];
        if (r >= 0 && (int64_t)r < n) assign[r] = (int32_t)grp_list_of_pos(off, L, pos);
    }
}

// a build's nearest-centroid ids as the canonical assignment: a row no
// centroid took goes to list 0, a row with an empty array to no list
__global__ __launch_bounds__(256) void k_grp_canon(const int64_t *assign, int64_t n, int64_t L,
                                                   const uint8_t *nonempty, int32_t *out) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t a = assign ? assign[i] : 0;
        out[i] = (nonempty && !bit_test(nonempty, i)) ? -1 : (a < 0 || a >= L) ? 0 : (int32_t)a;
    }
}

static int grp_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 65536); }

void launch_grp_count(const int32_t *assign, int64_t n, int64_t L, const uint8_t *nonempty, bool allow_none, int *cnt,
                      int *status, hipStream_t s) {
    if (n > 0)
        hipLaunchKernelGGL(k_grp_count, dim3(grp_grid(n)), dim3(256), 0, s, assign, n, L, nonempty, allow_none ? 1 : 0,
                           cnt, status);
}

void launch_grp_scan(const int *cnt, int64_t L, int pad, int64_t *off, int64_t *info, const int *status,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_grp_scan, dim3(1), dim3(1024), 0, s, cnt, L, pad, off, info, status);
}

void launch_grp_scatter(const int32_t *assign, int64_t n, int64_t L, const uint8_t *nonempty, const int64_t *off,
                        int *fill, int32_t *perm, hipStream_t s) {
    if (n > 0)
        hipLaunchKernelGGL(k_grp_scatter, dim3(grp_grid(n)), dim3(256), 0, s, assign, n, L, nonempty, off, fill, perm);
}

int32_t *launch_grp_sort(int32_t *perm, int32_t *tmp, const int64_t *off, const int *cnt, int64_t L, int64_t npos,
                         int64_t max_rows, hipStream_t s) {
    if (npos <= 0 || max_rows < 2) return perm;
    const int64_t runs = (max_rows + kSortCap - 1) / kSortCap;
    hipLaunchKernelGGL(k_grp_sort, dim3((unsigned)std::min<int64_t>(L, 2048), (unsigned)std::min<int64_t>(runs, 128)),
                       dim3(256), 0, s, perm, off, cnt, L);
    int32_t *src = perm, *dst = tmp;
    for (int64_t w = kSortCap; w < max_rows; w *= 2) {
        hipLaunchKernelGGL(k_grp_merge, dim3(grp_grid(npos)), dim3(256), 0, s, src, dst, off, cnt, L, npos, w);
        std::swap(src, dst);
    }
    return src;
}

void launch_grp_assign_of(const int32_t *perm, const int64_t *off, int64_t L, int64_t npos, int64_t n,
                          int32_t *assign, hipStream_t s) {
    if (npos > 0)
        hipLaunchKernelGGL(k_grp_assign_of, dim3(grp_grid(npos)), dim3(256), 0, s, perm, off, L, npos, n, assign);
}

void launch_grp_canon(const int64_t *assign, int64_t n, int64_t L, const uint8_t *nonempty, int32_t *out,
                      hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_grp_canon, dim3(grp_grid(n)), dim3(256), 0, s, assign, n, L, nonempty, out);
}


}  // namespace mqvs
