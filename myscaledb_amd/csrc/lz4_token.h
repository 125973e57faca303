// lz4_token.h -- the sequence grammar of the LZ4 block format (LZ4_decompress_
// faster.cpp:480-640), once: every parse of k_decode_blocks (kernels_lz4.hip)
// goes through lz4_parse and every sequence it runs through lz4_fits, so the
// guards between a malformed stream and a stray store stand here only.  Plain
// C++17 that a host compiler takes as well (tests/lz4_token_host.cpp).
// A byte reader is a functor `uint32_t operator()(int32_t pos)` over the
// block's compressed stream; it is called only with 0 <= pos < isz.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define LZ4_FN __host__ __device__ __forceinline__
#else
#define LZ4_FN inline
#endif

namespace mqvs {

struct Lz4Seq {
    int32_t lip, ll;  // the literals: position in the stream, length
    int32_t off, ml;  // the match: offset back from its output position, length (0, 0 when last)
    bool last;        // the literals-only final sequence: its literals end the stream
    int32_t next;     // position of the next token
};

// A length code of 15 goes on in the bytes at q: 255s, then the remainder.
// Lengths are cut off at 2^30 (larger blocks are refused as malformed).
template <class Reader>
LZ4_FN bool lz4_extend(Reader &rd, int32_t isz, int32_t &q, int32_t &len) {
    uint32_t b;
    do {
        if (q >= isz) return false;
        b = rd(q++);
        len += (int32_t)b;
    } while (b == 255 && len < (1 << 30));
    return true;
}

// The sequence whose token is at p < isz; false when it runs past the stream.
template <class Reader>
LZ4_FN bool lz4_parse(Reader &rd, int32_t p, int32_t isz, Lz4Seq &s) {
    const uint32_t t = rd(p);
    int32_t q = p + 1;
    s.ll = (int32_t)(t >> 4);
    if (s.ll == 15 && !lz4_extend(rd, isz, q, s.ll)) return false;
    if (s.ll > isz - q) return false;
    s.lip = q;
    q += s.ll;
    s.off = s.ml = 0;
    s.last = q == isz;
    if (!s.last) {
        if (isz - q < 2) return false;
        s.off = (int32_t)(rd(q) | (rd(q + 1) << 8));
        q += 2;
        s.ml = (int32_t)(t & 15);
        if (s.ml == 15 && !lz4_extend(rd, isz, q, s.ml)) return false;
        s.ml += 4;
    }
    s.next = q;
    return true;
}

// Whether sequence s, written at output position o, stays inside the block's
// output [0, osz) and reads only output before it.
LZ4_FN bool lz4_fits(const Lz4Seq &s, int32_t o, int32_t osz) {
    return !(s.ll > osz - o || (!s.last && (s.off == 0 || s.off > o + s.ll)) || s.ml > osz - o - s.ll);
}

}  // namespace mqvs
