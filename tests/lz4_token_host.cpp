// lz4_token_host.cpp -- the decoder's sequence grammar (csrc/lz4_token.h) on
// the CPU: a sequential LZ4 block decoder made of lz4_parse and lz4_fits alone,
// with the end-of-block rule of k_decode_blocks (the stream ends in the
// literals-only sequence and fills the output exactly).
//
//   lz4_token_host IN OUT
// IN:  per stream  int32 isz, int32 osz, isz compressed bytes
// OUT: per stream  int32 n (the decoded length osz, or -1: refused), n bytes
// (tests/test_lz4_token_host.py builds it, sanitizers on, and drives it.)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lz4_token.h"

struct VectorReader {
    const std::vector<uint8_t> &v;
    uint32_t operator()(int32_t pos) { return v.at((size_t)pos); }
};

static bool decode(const std::vector<uint8_t> &in, int32_t osz, std::vector<uint8_t> &out) {
    const int32_t isz = (int32_t)in.size();
    if (in.size() >= (1u << 30) || osz < 0 || osz >= (1 << 30)) return false;
    VectorReader rd{in};
    out.clear();
    for (int32_t p = 0; p < isz;) {
        mqvs::Lz4Seq s;
        const int32_t op = (int32_t)out.size();
        if (!mqvs::lz4_parse(rd, p, isz, s) || !mqvs::lz4_fits(s, op, osz)) return false;
        for (int32_t i = 0; i < s.ll; ++i) out.push_back(in.at((size_t)(s.lip + i)));
        if (s.last) return (int32_t)out.size() == osz;
        for (int32_t i = 0; i < s.ml; ++i) out.push_back(out.at(out.size() - (size_t)s.off));
        p = s.next;
    }
    return false;  // the stream ended in a match (or is empty)
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t hdr[2];
    std::vector<uint8_t> in, out;
    while (fread(hdr, sizeof(int32_t), 2, fi) == 2) {
        if (hdr[0] < 0) return 2;
        in.resize((size_t)hdr[0]);
        if (fread(in.data(), 1, in.size(), fi) != in.size()) return 2;
        const int32_t n = decode(in, hdr[1], out) ? hdr[1] : -1;
        fwrite(&n, sizeof n, 1, fo);
        if (n > 0) fwrite(out.data(), 1, (size_t)n, fo);
    }
    return fclose(fo) == 0 ? 0 : 2;
}
