// fp8_mfma_probe.hip -- how v_mfma_f32_16x16x32_fp8_fp8 (OCP e4m3fn operands)
// sums the 32 products of one instruction on gfx950, and what
// v_cvt_pk_fp8_f32 / v_cvt_scalef32_pk_bf16_fp8 do at the edges of the format.
// Why the fp8 list scan (k_ivf_scan_fp8, kernels_ivf_scan.hip) widens its codes to
// bf16 and uses the bf16 MFMA: see the output kept in
// profiles/index_fp8/fp8_mfma_probe.log.
//
//   hipcc -O2 --offload-arch=gfx950 tools/fp8_mfma_probe.hip -o tools/bin/fp8_mfma_probe
//   tools/bin/fp8_mfma_probe
//
// 1. conversion: subnormal grid and midpoints, values around 448, non-finite
// 2. directed MFMA cases: subnormal codes; small products beside a large one
// 3. random blocks (C = 0): the error of one instruction against the exact sum
//    of its 32 products, relative to the largest product, to sum |p| and to
//    |a| |b|, for (0) Gaussian vectors scaled as the index scales them, (1)
//    uniformly random codes, (2) Gaussian values with a wide spread of scales
// 4. v_cvt_scalef32_pk_bf16_fp8 with scale 1 on all 256 codes
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// ---- 1, 2: conversion and directed cases
__global__ void k_cvt_a(const float *in, int n, unsigned *out) {
    int i = threadIdx.x;
    if (i < n) out[i] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(in[i], 0.f, 0, false) & 0xFFu;
}
__global__ void k_mfma_a(const unsigned char *A, const unsigned char *B, const float *Cin, float *D) {
    const int lane = threadIdx.x, l16 = lane & 15, c = lane >> 4;
    long a = 0, b = 0;
    for (int j = 0; j < 8; ++j) {
        a |= (long)A[l16 * 32 + 8 * c + j] << (8 * j);
        b |= (long)B[(8 * c + j) * 16 + l16] << (8 * j);
    }
    f32x4 acc;
    for (int r = 0; r < 4; ++r) acc[r] = Cin[(4 * c + r) * 16 + l16];
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[(4 * c + r) * 16 + l16] = acc[r];
}
static float val_a(unsigned c) {
    unsigned e = (c >> 3) & 15, m = c & 7;
    float v = e == 0 ? m * ldexpf(1.f, -9) : (e == 15 && m == 7) ? NAN : ldexpf(1.f + m / 8.f, (int)e - 7);
    return (c & 0x80) ? -v : v;
}
static int part_a() {
    std::vector<float> in;
    for (int m = 0; m <= 16; ++m) in.push_back(m * ldexpf(1.f, -10));  // subnormal grid + midpoints, up to 2^-6
    for (float x : {ldexpf(1.f, -11), ldexpf(1.f, -12), 0.017f, 1.0f, 1.0625f, 1.1875f, 240.f, 248.f, 448.f, 460.f, 464.f, 480.f, 1e30f, INFINITY, -INFINITY, NAN, -0.001953125f}) in.push_back(x);
    int n = (int)in.size();
    float *din; unsigned *dout;
    (void)hipMalloc(&din, n * 4); (void)hipMalloc(&dout, n * 4);
    (void)hipMemcpy(din, in.data(), n * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_cvt_a, dim3(1), dim3(64), 0, 0, din, n, dout);
    std::vector<unsigned> out(n);
    (void)hipMemcpy(out.data(), dout, n * 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < n; ++i) printf("cvt %.10g -> 0x%02x (%.10g)\n", in[i], out[i], val_a(out[i]));
    // MFMA cases: row i of A and column i of B make case i
    std::vector<unsigned char> A(16 * 32, 0), B(32 * 16, 0);
    std::vector<float> C(256, 0.f), D(256);
    auto setk = [&](int cs, int k, unsigned a, unsigned b) { A[cs * 32 + k] = a; B[k * 16 + cs] = b; };
    setk(0, 0, 0x01, 0x38);                   // 2^-9 * 1
    setk(1, 0, 0x01, 0x01);                   // 2^-18
    setk(2, 0, 0x07, 0x7E);                   // 7 2^-9 * 448
    setk(3, 0, 0x38, 0x03);                   // 1 * 3 2^-9 (subnormal in B)
    setk(4, 0, 0x78, 0x78);                   // 2^16 + 16 * 2^-8
    for (int k = 1; k <= 16; ++k) setk(4, k, 0x18, 0x18);
    for (int k = 1; k <= 16; ++k) setk(5, k, 0x18, 0x18);  // C = 2^16 + 16 * 2^-8
    C[5 * 16 + 5] = 65536.f;
    setk(6, 0, 0x78, 0x78);                   // 2^16 + 2^-9 * 2^-2 ... + one product 2^-6
    setk(6, 1, 0x28, 0x10);                   // 2^-2 * 2^-5 = 2^-7 (one fp32 ulp of 2^16)
    setk(7, 0, 0x78, 0x78);                   // 2^16 + 31 * 2^-7
    for (int k = 1; k < 32; ++k) setk(7, k, 0x28, 0x10);
    setk(8, 0, 0x78, 0xF8);                   // 2^16 - 2^16 + 2^-18
    setk(8, 1, 0x78, 0x78);
    setk(8, 2, 0x01, 0x01);
    unsigned char *dA, *dB; float *dC, *dD;
    (void)hipMalloc(&dA, A.size()); (void)hipMalloc(&dB, B.size()); (void)hipMalloc(&dC, 1024); (void)hipMalloc(&dD, 1024);
    (void)hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice);
    (void)hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
    (void)hipMemcpy(dC, C.data(), 1024, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_mfma_a, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD);
    if (hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost) != hipSuccess) { printf("mfma kernel failed\n"); return 1; }
    const double expect[9] = {ldexp(1., -9), ldexp(1., -18), 7 * ldexp(1., -9) * 448, 3 * ldexp(1., -9), 65536 + 16 * ldexp(1., -8),
                              65536 + 16 * ldexp(1., -8), 65536 + ldexp(1., -7), 65536 + 31 * ldexp(1., -7), ldexp(1., -18)};
    for (int i = 0; i < 9; ++i) printf("mfma case %d: got %.12g expect %.12g\n", i, D[i * 16 + i], expect[i]);
    return 0;
}

// ---- 3: random blocks
__global__ void k_mfma_b(const unsigned char *A, const unsigned char *B, float *D, int nblk) {
    const int lane = threadIdx.x, l16 = lane & 15, c = lane >> 4;
    for (int t = blockIdx.x; t < nblk; t += gridDim.x) {
        const unsigned char *a8 = A + (size_t)t * 512, *b8 = B + (size_t)t * 512;
        long a = 0, b = 0;
        for (int j = 0; j < 8; ++j) {
            a |= (long)a8[l16 * 32 + 8 * c + j] << (8 * j);
            b |= (long)b8[l16 * 32 + 8 * c + j] << (8 * j);   // B stored [col][k]
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc, 0, 0, 0);
        for (int r = 0; r < 4; ++r) D[(size_t)t * 256 + (4 * c + r) * 16 + l16] = acc[r];
    }
}
static double val_b(unsigned c) {
    unsigned e = (c >> 3) & 15, m = c & 7;
    double v = e == 0 ? m * ldexp(1., -9) : ldexp(1. + m / 8., (int)e - 7);
    return (c & 0x80) ? -v : v;
}
static unsigned enc_b(double x) {  // RNE to e4m3fn, |x| < 448
    unsigned best = 0; double bd = 1e300;
    for (unsigned c = 0; c < 0x7F; ++c) { double d = fabs(fabs(x) - val_b(c)); if (d < bd || (d == bd && !(c & 1))) { bd = d; best = c; } }
    return best | (x < 0 ? 0x80 : 0);
}
static int part_b() {
    const int nblk = 4096;
    std::mt19937 rng(12345);
    std::normal_distribution<double> nd(0, 1);
    for (int mode = 0; mode < 3; ++mode) {
        std::vector<unsigned char> A((size_t)nblk * 512), B((size_t)nblk * 512);
        for (int t = 0; t < nblk; ++t)
            for (int r = 0; r < 16; ++r) {
                // mode 0: gaussian vectors scaled so that |max| is in [128, 256) (the index's quantiser)
                // mode 1: any code, uniformly; mode 2: gaussian with a log-uniform scale per element (wide spread)
                double va[32], vb[32], ma = 0, mb = 0;
                for (int k = 0; k < 32; ++k) {
                    va[k] = nd(rng); vb[k] = nd(rng);
                    if (mode == 2) { va[k] *= ldexp(1., -(int)(rng() % 12)); vb[k] *= ldexp(1., -(int)(rng() % 12)); }
                    ma = fmax(ma, fabs(va[k])); mb = fmax(mb, fabs(vb[k]));
                }
                int ea, eb; frexp(ma, &ea); frexp(mb, &eb);
                for (int k = 0; k < 32; ++k) {
                    if (mode == 1) {
                        unsigned ca = rng() & 0xFF, cb = rng() & 0xFF;
                        if ((ca & 0x7F) == 0x7F) ca = 0; if ((cb & 0x7F) == 0x7F) cb = 0;
                        A[(size_t)t * 512 + r * 32 + k] = ca; B[(size_t)t * 512 + r * 32 + k] = cb;
                    } else {
                        A[(size_t)t * 512 + r * 32 + k] = enc_b(ldexp(va[k], 8 - ea));
                        B[(size_t)t * 512 + r * 32 + k] = enc_b(ldexp(vb[k], 8 - eb));
                    }
                }
            }
        unsigned char *dA, *dB; float *dD;
        if (hipMalloc(&dA, A.size()) != hipSuccess || hipMalloc(&dB, B.size()) != hipSuccess || hipMalloc(&dD, (size_t)nblk * 1024) != hipSuccess) return 2;
        (void)hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice);
        (void)hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_mfma_b, dim3(256), dim3(64), 0, 0, dA, dB, dD, nblk);
        std::vector<float> D((size_t)nblk * 256);
        if (hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
        double wmax = 0, wsum = 0, wl2 = 0; long neg = 0, pos = 0, zero = 0, towardzero = 0, away = 0;
        for (int t = 0; t < nblk; ++t)
            for (int i = 0; i < 16; ++i)
                for (int j = 0; j < 16; ++j) {
                    double s = 0, sa = 0, mx = 0, na = 0, nb = 0;
                    for (int k = 0; k < 32; ++k) {
                        double x = val_b(A[(size_t)t * 512 + i * 32 + k]), y = val_b(B[(size_t)t * 512 + j * 32 + k]);
                        s += x * y; sa += fabs(x * y); mx = fmax(mx, fabs(x * y)); na += x * x; nb += y * y;
                    }
                    double got = D[(size_t)t * 256 + i * 16 + j], err = got - s;
                    // (exact sum rounded to fp32 would differ by at most half an ulp: ignore that much)
                    double ulp = ldexp(1., (int)floor(log2(fmax(fabs(s), 1e-300))) - 23);
                    if (fabs(err) <= ulp / 2) { ++zero; continue; }
                    (err < 0 ? neg : pos)++;
                    ((fabs(got) < fabs(s)) ? towardzero : away)++;
                    if (mx > 0) wmax = fmax(wmax, fabs(err) / mx);
                    if (sa > 0) wsum = fmax(wsum, fabs(err) / sa);
                    if (na * nb > 0) wl2 = fmax(wl2, fabs(err) / sqrt(na * nb));
                }
        printf("mode %d: worst |err|/max|p| = 2^%.2f, |err|/sum|p| = 2^%.2f, |err|/(|a||b|) = 2^%.2f; within half ulp %ld, below %ld, above %ld, toward zero %ld, away %ld\n",
               mode, log2(wmax), log2(wsum), log2(wl2), zero, neg, pos, towardzero, away);
        (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dD);
    }
    return 0;
}

// ---- 4: fp8 -> bf16
__global__ void k_c(unsigned *o) {
    const unsigned c = threadIdx.x;  // 256 threads
    const unsigned lo = c | ((c ^ 0x5Au) << 8), word = lo | (lo << 16);
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, true);
    o[2 * c] = __builtin_bit_cast(unsigned, a);
    o[2 * c + 1] = __builtin_bit_cast(unsigned, b);
}
static float val_c(unsigned c) {
    unsigned e = (c >> 3) & 15, m = c & 7;
    float v = e == 0 ? m * ldexpf(1.f, -9) : (e == 15 && m == 7) ? NAN : ldexpf(1.f + m / 8.f, (int)e - 7);
    return (c & 0x80) ? -v : v;
}
static float bf_c(unsigned h) { unsigned u = h << 16; float f; memcpy(&f, &u, 4); return f; }
static int part_c() {
    unsigned *d, h[512];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
    hipLaunchKernelGGL(k_c, dim3(1), dim3(256), 0, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    int bad = 0;
    for (unsigned c = 0; c < 256; ++c)
        for (int w = 0; w < 2; ++w) {
            const float e0 = val_c(c), e1 = val_c((c ^ 0x5A) & 0xFF);
            const float g0 = bf_c(h[2 * c + w] & 0xFFFF), g1 = bf_c(h[2 * c + w] >> 16);
            const bool ok0 = (e0 != e0) ? (g0 != g0) : (g0 == e0 && std::signbit(g0) == std::signbit(e0));
            const bool ok1 = (e1 != e1) ? (g1 != g1) : (g1 == e1 && std::signbit(g1) == std::signbit(e1));
            if (!ok0 || !ok1) { if (bad++ < 12) printf("code %02x sel %d: got (%g, %g) = %08x expect (%g, %g)\n", c, w, g0, g1, h[2 * c + w], e0, e1); }
        }
    printf("cvt_scalef32_pk_bf16_fp8: %d mismatches of 1024\n", bad);
    return 0;
}

int main() {
    int rc = part_a();
    if (rc == 0) rc = part_b();
    if (rc == 0) rc = part_c();
    return rc;
}
