// The spread of the i8 MFMA route (myscaledb_amd/csrc/binary_spread.h) against
// its definition, for every 16-bit input: byte i of the 16 output bytes is bit
// i of the input.  Host code only; tests/test_binary_expand.py builds and runs it.
#include <cstdio>
#include <cstring>

#include "binary_spread.h"

int main() {
    long bad = 0;
    for (uint32_t v = 0; v < 65536u; ++v) {
        // bits above the low 16 must be ignored
        const uint32_t inputs[2] = {v, v | 0xABCD0000u};
        for (uint32_t in : inputs) {
            uint32_t out[4];
            bin_spread16(in, out);
            unsigned char bytes[16];
            std::memcpy(bytes, out, 16);
            for (int i = 0; i < 16; ++i) {
                // (little-endian words: byte i of the 16 is byte i % 4 of word i / 4)
                const unsigned want = (v >> i) & 1u;
                const unsigned got_word = (out[i / 4] >> (8 * (i % 4))) & 0xFFu;
                if (got_word != want || bytes[i] != want) {
                    if (bad < 5) std::printf("input %#x byte %d: %u, expected %u\n", in, i, got_word, want);
                    ++bad;
                }
            }
        }
    }
    for (uint32_t nib = 0; nib < 16u; ++nib) {
        const uint32_t w = bin_spread4(nib);
        for (int i = 0; i < 4; ++i)
            if (((w >> (8 * i)) & 0xFFu) != ((nib >> i) & 1u)) ++bad;
    }
    std::printf("checked 65536 inputs, %ld mismatches\n", bad);
    return bad ? 1 : 0;
}
