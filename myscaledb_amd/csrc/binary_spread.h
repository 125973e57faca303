// binary_spread.h -- bits of a binary code as 0/1 bytes, the operand form of
// the i8 MFMA route (kernels_binary_mfma.hip).  Rows and columns of a product
// go through this one function, so their k order agrees by construction.
// Pure integer code: a plain C++ compiler takes it too (tests/test_binary_expand.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MQVS_SPREAD_HD __host__ __device__
#else
#define MQVS_SPREAD_HD
#endif

// byte i of the result = bit i of nib (nib < 16).  Two shift-ors copy bit i to
// positions i, i + 7, i + 14, i + 21 -- all distinct over i = 0 .. 3 -- and the
// mask keeps positions 0, 8, 16, 24, which are bits 0, 1, 2, 3.
MQVS_SPREAD_HD inline uint32_t bin_spread4(uint32_t nib) {
    uint32_t t = nib | (nib << 7);
    t |= t << 14;
    return t & 0x01010101u;
}

// byte i of the 16 bytes out[0 .. 3] (little endian) = bit i of bits (its
// low 16 bits; the rest is ignored)
MQVS_SPREAD_HD inline void bin_spread16(uint32_t bits, uint32_t (&out)[4]) {
    out[0] = bin_spread4(bits & 15u);
    out[1] = bin_spread4((bits >> 4) & 15u);
    out[2] = bin_spread4((bits >> 8) & 15u);
    out[3] = bin_spread4((bits >> 12) & 15u);
}
