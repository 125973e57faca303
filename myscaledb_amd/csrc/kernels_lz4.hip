// kernels_lz4.hip -- the LZ4 block decoder of the column ingest (segment.hip)
// and of the index blob reader (index_blob.hip): k_decode_blocks, one 64-lane
// workgroup per block (LZ4_decompress_faster.cpp:480-640 block format).  The
// sequence grammar and its guards are lz4_token.h; how the wave parses and
// runs the sequences stands above kChunk below.
#include "flat_kernels.h"
#include "lz4_token.h"

namespace mqvs {

// LDS ring of the block's latest output.  4 KiB (not the 64 KiB LZ4 window)
// so that twelve decode waves fit on a CU (three per SIMD): the
// decode is latency-bound per wave, and a 64 KiB ring left two waves per CU.
// Matches reaching further back (~6 % of them on quantised float columns)
// read the already-flushed output from global memory (far_byte).
constexpr int kRing = 4096;
constexpr int kFlush = 1024;  // unflushed output < kFlush + one step (< kRing - 256)
// a group holds sequences of at most kGrpLit literals and kGrpMatch match
// bytes: 64 of them write < kRing - kFlush - 256 bytes
constexpr int kGrpLit = 16, kGrpMatch = 27;
static_assert(64 * (kGrpLit + kGrpMatch) + kFlush + 256 < kRing, "group output must fit the ring");

// The dword at a + q (a dword-aligned), of a stream that ends at a + lim:
// only the bytes before the end are read, the others are 0.
template <class I>
__device__ __forceinline__ uint32_t dword_clamped(const uint8_t *a, I q, I lim) {
    if (q + 4 <= lim) return *reinterpret_cast<const uint32_t *>(a + q);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (q + k < lim) v |= (uint32_t)a[q + k] << (8 * k);
    return v;
}

// Literal run: output bytes [op, op + len) of the block <- s[0, len), also
// into the LDS ring.  Long runs (incompressible floats are one run per block)
// go by whole output dwords: two aligned source dwords per lane joined by
// v_alignbyte, 8 per lane in flight (2 KiB per wave); the ragged head and tail
// go byte by byte.  out must be 4-byte aligned for the dword path.
__device__ __forceinline__ void copy_literals(const uint8_t *s, const uint8_t *s_end, uint8_t *out, int64_t op,
                                              int64_t len, uint8_t *ring, int lane) {
    auto byte_copy = [&](int64_t b, int64_t e) {
        for (int64_t i = b + lane; i < e; i += 64) {
            const uint8_t v = s[i];
            out[op + i] = v;
            ring[(op + i) & (kRing - 1)] = v;
        }
    };
    if (len < 256 || ((uintptr_t)out & 3)) {
        byte_copy(0, len);
        return;
    }
    const int64_t head = (4 - (op & 3)) & 3;
    byte_copy(0, head);
    const int64_t p0 = op + head, nw = (len - head) >> 2;
    const uintptr_t sa = (uintptr_t)(s + head);
    const int sh = (int)(sa & 3);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(sa & ~(uintptr_t)3);
    const int64_t sw_lim = s_end - (const uint8_t *)sw;
    uint32_t *ow = reinterpret_cast<uint32_t *>(out + p0);
    uint32_t *rw = reinterpret_cast<uint32_t *>(ring);
    const int64_t r0 = p0 >> 2;
    constexpr int U = 8;
    for (int64_t w0 = 0; w0 < nw; w0 += 64 * U) {
        uint32_t lo[U], hi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t w = w0 + u * 64 + lane;
            lo[u] = hi[u] = 0;
            if (w < nw) {
                lo[u] = sw[w];
                if (sh) hi[u] = dword_clamped((const uint8_t *)sw, 4 * (w + 1), sw_lim);  // the stream may end in it
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t w = w0 + u * 64 + lane;
            if (w < nw) {
                const uint32_t v = sh ? __builtin_amdgcn_alignbyte(hi[u], lo[u], (uint32_t)sh) : lo[u];
                ow[w] = v;
                rw[(r0 + w) & (kRing / 4 - 1)] = v;
            }
        }
    }
    byte_copy(head + 4 * nw, len);
}

// A byte of this wave's own earlier, flushed output: the stores are waited
// for (vmcnt) by the caller; the load bypasses the non-coherent L1 (agent-
// scope atomic load of the containing dword).
__device__ __forceinline__ uint32_t far_byte(const uint8_t *out, int32_t pos) {
    const uintptr_t a = (uintptr_t)(out + pos);
    const uint32_t w = __hip_atomic_load(reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    return (w >> (8 * (a & 3))) & 255u;
}

// The decoder stages a block's compressed bytes in LDS kChunk at a time (plus
// kLook bytes of look-ahead) and parses each chunk with all 64 lanes: the
// chunk is cut into 64 segments of kSeg bytes and lane i parses the tokens
// that START in segment i.  A lane cannot know where its first token starts,
// so it first parses speculatively from each of the segment's first kStarts
// bytes (pass A), recording each parse's first kSpec token positions with the
// output / record counts before them: an LZ4 parse started at an arbitrary
// byte mostly falls into the true token chain within a few tokens.  A uniform walk over the 64 lanes then
// chains the true entries -- segment i's entry is segment i-1's exit; when
// the entry is among lane i's recorded positions its exit and counts follow,
// otherwise the segment is re-parsed from the entry right there -- and each
// lane re-parses its segment from its true entry (pass B), writing one record
// per sequence (literal position and length, offset, match length, output
// position) to LDS.  The records then run in order, up to 64 at a time, one
// lane per sequence: every literal run at once (they depend on nothing), then
// the matches in rounds -- a match is copied in the first round in which no
// unfinished match before it writes its source bytes (the first unfinished
// one always can be), so each round makes progress.  A match reads
// byte src + (t mod off) for output byte t, so the replication of an
// overlapping match (off < length) needs no ordering of its own.  Sequences
// longer than kGrpLit / kGrpMatch end a group and take wave-wide paths.
// (The round-2 decoder parsed tokens one at a time in scalar registers: ~500
// cycles per sequence on quantised floats, 0.25 s for a 3 GB column.)
//
// Output goes to an LDS ring only and is flushed to global memory in runs of
// >= kFlush bytes with dword stores; unflushed bytes stay < kFlush + one
// group, so the ring never overwrites them and every byte further back than
// the ring is already in global memory (far matches read it there).  (One
// wave per workgroup: its LDS accesses complete in program order, so a read
// after a write sees it; the wave barriers only keep the compiler from moving
// them.)  Positions are 32-bit (larger blocks are rejected as malformed).
constexpr int kChunk = 1024, kLook = 256, kSeg = kChunk / 64, kSpec = 4, kStarts = 4;
constexpr int kMaxRec = kChunk / 3 + 2;  // tokens starting in a chunk (>= 3 bytes each but the last)
constexpr int kCinWords = (kChunk + kLook) / 4 + 2;

// The wave's state for the block it decodes.
struct Decoder {
    uint8_t *ring;                      // LDS: the block's latest kRing output bytes
    uint32_t *cinw;                     // LDS: the staged chunk, kCinWords dwords,
    const uint8_t *cin;                 //      and the same as bytes
    uint4 *recs;                        // LDS: a chunk's records (literal position, output position, ll, ml)
    uint16_t *roff;                     //      and their offsets
    const uint8_t *ip0, *pa, *src_end;  // the stream; pa = ip0 - mis, dword-aligned; the end of the whole source
    uint8_t *out;                       // the block's output
    int32_t mis, isz, osz, lim;         // stream bytes at pa[mis, lim = mis + isz); osz output bytes
    int32_t cb, clen;                   // LDS holds pa bytes [cb, cb + clen)
    int32_t fl, op;                     // out[0, fl) written; output in the ring so far (uniform)
    int lane;

    __device__ __forceinline__ void begin(const uint8_t *ip, uint8_t *o, int32_t isz_, int32_t osz_) {
        ip0 = ip, out = o, isz = isz_, osz = osz_;
        mis = (int32_t)((uintptr_t)ip0 & 3);
        pa = ip0 - mis, lim = mis + isz;
        cb = clen = fl = op = 0;
    }
    __device__ __forceinline__ uint8_t &ring_at(int32_t pos) const { return ring[pos & (kRing - 1)]; }
    // byte `pos` of the block's compressed stream (per lane; pos < isz): staged, or from global memory
    __device__ __forceinline__ uint32_t operator()(int32_t pos) const {
        const int32_t r = mis + pos - cb;
        return (r >= 0 && r < clen) ? (uint32_t)cin[r] : (uint32_t)ip0[pos];
    }
    // out[fl, upto) <- the ring, by dwords
    __device__ __forceinline__ void flush(int32_t upto) {
        const int32_t oa = (int32_t)((uintptr_t)(out + fl) & 3);
        int32_t head = (4 - oa) & 3;
        if (head > upto - fl) head = upto - fl;
        if (lane < head) out[fl + lane] = ring_at(fl + lane);
        const int32_t p0 = fl + head, nw = (upto - p0) >> 2;
        uint32_t *ow = reinterpret_cast<uint32_t *>(out + p0);
        for (int32_t w = lane; w < nw; w += 64) {
            const int32_t b = p0 + 4 * w;
            ow[w] = (uint32_t)ring_at(b) | ((uint32_t)ring_at(b + 1) << 8) | ((uint32_t)ring_at(b + 2) << 16) |
                    ((uint32_t)ring_at(b + 3) << 24);
        }
        const int32_t p1 = p0 + 4 * nw;
        if (lane < upto - p1) out[p1 + lane] = ring_at(p1 + lane);
        fl = upto;
    }
    // a long sequence (wave-wide): literals [lip, lip + len) at op ...
    __device__ __forceinline__ void long_literals(int32_t lip, int32_t len) {
        if (len > 256) {
            flush(op);
            copy_literals(ip0 + lip, src_end, out, op, len, ring, lane);
            fl = op + len;
        } else {
            for (int32_t r = 0; r < len; r += 64)
                if (r + lane < len) ring_at(op + r + lane) = (uint8_t)(*this)(lip + r + lane);
        }
        op += len;
    }
    // ... then its match, 256 bytes per step
    __device__ __forceinline__ void long_match(int32_t off, int32_t mlen) {
        for (int32_t d0 = 0; d0 < mlen; d0 += 256) {
            const int32_t cnt = mlen - d0 < 256 ? mlen - d0 : 256, at = op + d0;
            __builtin_amdgcn_wave_barrier();
            if (at - fl >= kFlush) {
                flush(at);
                __builtin_amdgcn_wave_barrier();
            }
            uint32_t v[4];
            if (off > kRing - 256) {
                // far match (off > mlen-step, so no replication within a
                // 256-byte step): from the flushed output
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the flushes landed)
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = u * 64 + lane < cnt ? far_byte(out, at + u * 64 + lane - off) : 0u;
                __builtin_amdgcn_wave_barrier();
            } else {
                // byte op + i equals byte op + i - m off for any m >= 1, so step
                // [d0, d0 + cnt) reads the latest off bytes before it, all final
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int32_t i = u * 64 + lane;
                    v[u] = i < cnt ? (uint32_t)ring_at(at + i - (i / off + 1) * off) : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u * 64 + lane < cnt) ring_at(at + u * 64 + lane) = (uint8_t)v[u];
        }
        __builtin_amdgcn_wave_barrier();
        op += mlen;
    }
};

// The speculative parse's reader: staged bytes only (a parse inside a long literal run must not chase
// global memory).  A byte outside them reads as 0 and sets `miss`: such a parse is not the true chain.
struct StagedReader {
    const Decoder &d;
    bool miss = false;
    __device__ __forceinline__ uint32_t operator()(int32_t pos) {
        const int32_t r = d.mis + pos - d.cb;
        if (r >= 0 && r < d.clen) return (uint32_t)d.cin[r];
        miss = true;
        return 0u;
    }
};

// The token path's reader: a 256-B window of the stream held one dword per
// lane; uniform pos in, uniform byte out (v_readlane).
struct WindowReader {
    const Decoder &d;
    int32_t wa = -(1 << 30);
    uint32_t wv = 0;
    __device__ __forceinline__ uint32_t operator()(int32_t pos) {
        const int32_t x = d.mis + pos;
        if (x < wa || x >= wa + 256) {
            wa = x & ~3;
            wv = dword_clamped(d.pa, wa + 4 * d.lane, d.lim);
            wa = __builtin_amdgcn_readfirstlane(wa);
        }
        const int32_t o = x - wa;
        return ((uint32_t)__builtin_amdgcn_readlane((int)wv, o >> 2) >> (8 * (o & 3))) & 255u;
    }
};

// Nearly incompressible blocks (ratio below 8/7: a few long literal runs,
// e.g. 167 sequences of ~6 KB per MiB of Gaussian floats): the tokens one at
// a time, uniformly, through the window -- the chunked parse would stage and
// parse a chunk per token.  True when the final sequence was reached.  (A
// sequence is parsed and checked whole, match included, before its literals go.)
__device__ __forceinline__ bool decode_by_token(Decoder &d) {
    WindowReader rd{d};
    for (int32_t p = 0; p < d.isz;) {
        p = __builtin_amdgcn_readfirstlane(p);
        d.op = __builtin_amdgcn_readfirstlane(d.op);
        d.fl = __builtin_amdgcn_readfirstlane(d.fl);
        Lz4Seq s;
        if (!lz4_parse(rd, p, d.isz, s) || !lz4_fits(s, d.op, d.osz)) return false;
        if (d.op - d.fl >= kFlush) d.flush(d.op);
        d.long_literals(s.lip, s.ll);
        if (s.last) return true;
        d.long_match(s.off, s.ml);
        if (d.op - d.fl >= kFlush) d.flush(d.op);
        p = s.next;
    }
    return false;  // the stream ended in a match
}

// ---- stage [cs, cs + kChunk + kLook) of the stream
__device__ __forceinline__ void stage_chunk(Decoder &d, int32_t cs) {
    __builtin_amdgcn_wave_barrier();
    d.cb = (d.mis + cs) & ~3;
    d.clen = d.lim - d.cb < kChunk + kLook + 4 ? d.lim - d.cb : kChunk + kLook + 4;
    constexpr int kStageW = (kChunk + kLook) / 256 + 1;
    uint32_t v[kStageW];
#pragma unroll
    for (int u = 0; u < kStageW; ++u) v[u] = dword_clamped(d.pa, d.cb + 4 * (u * 64 + d.lane), d.lim);
#pragma unroll
    for (int u = 0; u < kStageW; ++u)
        if (u * 64 + d.lane < kCinWords) d.cinw[u * 64 + d.lane] = v[u];
    __builtin_amdgcn_wave_barrier();
}

// What a lane's parse from start c of its segment found: its first kSpec token
// positions rp with the output counts rc before them, where it left the segment
// (xs; -1: it ran off the stream), its output count ts and its token count ns.
struct SpecParse {
    int32_t rp[kStarts][kSpec], rc[kStarts][kSpec], xs[kStarts], ts[kStarts], ns[kStarts];
};

// ---- pass A: speculative parses of the segment from its first kStarts bytes
// (one start per byte: on quantised floats, tokens of 3 bytes, a parse started
// in the wrong byte phase stays in it -- offsets below 4096 read as tokens
// without literals -- and missed the true chain for 2 of 3 segments; from 4
// starts the true entry is a start or a recorded position for 99.9 %)
__device__ __forceinline__ SpecParse parse_speculative(const Decoder &d, int32_t cs, int32_t E) {
    const int32_t s0 = cs + kSeg * d.lane, s1 = s0 + kSeg;  // this lane's segment
    SpecParse a;
#pragma unroll
    for (int c = 0; c < kStarts; ++c) {
        int32_t x = s0 + c, t = 0, nn = 0;
#pragma unroll
        for (int j = 0; j < kSpec; ++j) a.rp[c][j] = -1, a.rc[c][j] = 0;
        if (s1 > E) {
            while (x < s1 && x < d.isz) {
#pragma unroll
                for (int j = 0; j < kSpec; ++j) {  // (selects: no branches in this loop)
                    a.rp[c][j] = nn == j ? x : a.rp[c][j];
                    a.rc[c][j] = nn == j ? t : a.rc[c][j];
                }
                StagedReader rd{d};
                Lz4Seq s;
                if (!lz4_parse(rd, x, d.isz, s) || rd.miss) {
                    x = -1;  // runs off the stream: not the true chain
                    break;
                }
                t += s.ll + s.ml;
                ++nn;
                x = s.next;
                if (s.last) break;
            }
        }
        a.xs[c] = x;
        a.ts[c] = t;
        a.ns[c] = nn;
    }
    return a;
}

// The chain's result: per lane, the true entry of its segment with the output
// position and record index there; uniform, the chunk's record count R.
struct Chain {
    int32_t vE, vO, vR, R;
    bool bad;
};

// ---- the true chain over the segments (uniform): E, the next true token
// position, moves on to the first one past the chunk (segments without a true
// token start keep vE = isz: no pass B; the walk visits only the segments the
// chain enters)
__device__ __forceinline__ Chain walk_chain(const Decoder &d, const SpecParse &a, int32_t cs, int32_t &Eio) {
    // (plain locals: as members of the result the compiler took the loop's condition for divergent)
    const int32_t isz = d.isz;
    int32_t vE = isz, vO = 0, vR = 0, R = 0, O = d.op, E = Eio;
    bool bad = false;
    for (int i = (E - cs) / kSeg; i < 64 && E < isz && !bad; i = (E - cs) / kSeg) {
        const int32_t si = cs + kSeg * i, ei = si + kSeg;
        vE = d.lane == i ? E : vE;
        vO = d.lane == i ? O : vO;
        vR = d.lane == i ? R : vR;
        bool hit = false;
        const int32_t dl = E - si;
        if (dl < kStarts) {
            // the common case: a parse started at the entry
            int32_t hx = -1, ht = 0, hn = 0;
#pragma unroll
            for (int c = 0; c < kStarts; ++c)
                if (c == dl) {
                    hx = __builtin_amdgcn_readlane(a.xs[c], i);
                    ht = __builtin_amdgcn_readlane(a.ts[c], i);
                    hn = __builtin_amdgcn_readlane(a.ns[c], i);
                }
            if (hx >= 0) {
                hit = true;
                O += ht;
                R += hn;
                E = hx;
            }
        }
        if (!hit) {
            // a later recorded position of some parse
#pragma unroll
            for (int c = 0; c < kStarts; ++c)
#pragma unroll
                for (int j = 1; j < kSpec; ++j) {
                    if (hit) continue;
                    const int32_t nc = __builtin_amdgcn_readlane(a.ns[c], i);
                    const int32_t xc = __builtin_amdgcn_readlane(a.xs[c], i);
                    if (j < nc && xc >= 0 && __builtin_amdgcn_readlane(a.rp[c][j], i) == E) {
                        hit = true;
                        O += __builtin_amdgcn_readlane(a.ts[c], i) - __builtin_amdgcn_readlane(a.rc[c][j], i);
                        R += nc - j;
                        E = xc;
                    }
                }
        }
        if (!hit) {
            // no parse met the entry: re-parse the segment here (uniform arguments: every lane computes the same)
            int32_t p = E;
            while (p < ei && p < isz) {
                Lz4Seq s;
                if (!lz4_parse(d, p, isz, s)) {
                    bad = true;
                    break;
                }
                O += s.ll + s.ml;
                ++R;
                p = __builtin_amdgcn_readfirstlane(s.next);
                if (s.last) break;
            }
            E = p;
        }
        E = __builtin_amdgcn_readfirstlane(E);
        O = __builtin_amdgcn_readfirstlane(O);
        R = __builtin_amdgcn_readfirstlane(R);
    }
    Eio = E;
    return Chain{vE, vO, vR, R, bad};
}

// ---- pass B: records from the true entries; false when a lane met a
// sequence that is malformed or does not fit the output
__device__ __forceinline__ bool write_records(const Decoder &d, int32_t cs, const Chain &ch) {
    const int32_t s1 = cs + kSeg * (d.lane + 1);
    bool lbad = false;
    int32_t p = ch.vE, o = ch.vO, r = ch.vR;
    while (p < s1 && p < d.isz) {
        Lz4Seq s;
        if (!lz4_parse(d, p, d.isz, s) || !lz4_fits(s, o, d.osz) || r >= kMaxRec) {
            lbad = true;
            break;
        }
        d.recs[r] = uint4{(uint32_t)s.lip, (uint32_t)o, (uint32_t)s.ll, (uint32_t)s.ml};
        d.roff[r] = (uint16_t)s.off;
        ++r;
        o += s.ll + s.ml;
        p = s.next;
        if (s.last) break;
    }
    return __ballot(lbad) == 0;
}

// This lane's record of a run: x literal position, y output position, z ll, w ml
struct LaneRec {
    uint4 rec;
    int32_t off;
};

// ---- run records [r0, r0 + g), a lane each: the group's literals, then its
// matches in dependency rounds
__device__ __forceinline__ void run_group(Decoder &d, const LaneRec &lr, int g) {
    const uint4 rec = lr.rec;
    const int32_t off = lr.off, lane = d.lane;
    const bool act = lane < g;
    const int32_t dst_ = (int32_t)rec.y;  // the sequence's literals
    const int32_t gl = act ? (int32_t)rec.z : 0, gm = act ? (int32_t)rec.w : 0;
    const int32_t mdst = dst_ + gl;  // its match
    const int32_t gend = __builtin_amdgcn_readlane(mdst + gm, g - 1);
    // literal runs (bytes of the staged input, mostly)
    for (int32_t t0 = 0; __ballot(gl > t0) != 0; t0 += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = t0 + u < gl ? d((int32_t)rec.x + t0 + u) : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + u < gl) d.ring_at(dst_ + t0 + u) = (uint8_t)v[u];
    }
    // bytes below far_lim may be overwritten in the ring by this group: they
    // come from the flushed output (all of it is: the unflushed tail is
    // < kFlush bytes behind the group's start)
    const int32_t far_lim = gend - kRing, srcp = mdst - off;
    const bool far = gm > 0 && srcp < far_lim;
    // far matches: their bytes, as dwords of the flushed output re-aligned to
    // the source (off > gm: no replication), loaded before the rounds
    uint32_t fw[kGrpMatch / 4 + 1];
#pragma unroll
    for (int i = 0; i < kGrpMatch / 4 + 1; ++i) fw[i] = 0;
    if (__ballot(far) != 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the flushes landed)
        const uintptr_t fa = (uintptr_t)(d.out + (far ? srcp : 0));
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(fa & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(fa & 3);
        uint32_t raw[kGrpMatch / 4 + 2];
#pragma unroll
        for (int i = 0; i < kGrpMatch / 4 + 2; ++i)
            raw[i] = far && 4 * i < gm + (int)sh ? __hip_atomic_load(wp + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                 : 0u;
#pragma unroll
        for (int i = 0; i < kGrpMatch / 4 + 1; ++i) fw[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
    }
    // A match is copied once no unfinished match writes its source bytes: the
    // lanes before it whose match ends past its source start (a binary search
    // over the lanes' ordered match ends), [kl, lane).  Literal bytes are all
    // written already.  (Sources before the group -- far ones included -- and
    // the replicated prefix of an overlapping match: no lanes.)
    const int32_t need_end = off < gm ? mdst : srcp + gm;
    const int32_t mend = mdst + gm;
    int kl = 0, kh = 0;  // lanes [kl, kh): match end > srcp, match start < need_end
#pragma unroll
    for (int st = 32; st >= 1; st >>= 1) {
        const int cl = kl + st - 1, ch = kh + st - 1;
        const int32_t el = __shfl(mend, cl < 64 ? cl : 63);
        const int32_t sh_ = __shfl(mdst, ch < 64 ? ch : 63);
        if (kl + st <= lane && el <= srcp) kl += st;
        if (kh + st <= lane && sh_ < need_end) kh += st;
    }
    auto below = [](int x) -> uint64_t { return x <= 0 ? 0ull : (~0ull >> (64 - x)); };
    const uint64_t deps = kh > kl ? below(kh) & ~below(kl) : 0ull;
    bool fin = gm == 0;
    while (true) {
        const uint64_t und = __ballot(!fin);
        if (und == 0) break;
        const bool go = !fin && (und & deps) == 0;
        if (go) {
            int32_t k = 0;  // (t mod off)
#pragma unroll
            for (int c = 0; c < (kGrpMatch + 11) / 12; ++c) {
                if (12 * c >= gm) break;
                uint32_t v[12];
#pragma unroll
                for (int u = 0; u < 12; ++u) {
                    const int t = 12 * c + u;
                    v[u] = 0;
                    if (t < gm) {
                        v[u] = far ? (fw[t >> 2] >> (8 * (t & 3))) & 255u : (uint32_t)d.ring_at(srcp + k);
                        k = k + 1 == off ? 0 : k + 1;
                    }
                }
#pragma unroll
                for (int u = 0; u < 12; ++u)
                    if (12 * c + u < gm) d.ring_at(mdst + 12 * c + u) = (uint8_t)v[u];
            }
        }
        fin = fin || go;
    }
    __builtin_amdgcn_wave_barrier();
    d.op = gend;
}

// ---- the long sequence at lane g, which ended the group
__device__ __forceinline__ void run_long(Decoder &d, const LaneRec &lr, int g) {
    const int32_t lip = __builtin_amdgcn_readlane((int)lr.rec.x, g), off = __builtin_amdgcn_readlane(lr.off, g);
    const int32_t ll = __builtin_amdgcn_readlane((int)lr.rec.z, g), ml = __builtin_amdgcn_readlane((int)lr.rec.w, g);
    if (d.op - d.fl >= kFlush) d.flush(d.op);
    d.long_literals(lip, ll);
    if (ml > 0) d.long_match(off, ml);
}

// ---- run a chunk's R records in order, up to 64 at a time
__device__ __forceinline__ void run_records(Decoder &d, int32_t R) {
    for (int32_t r0 = 0; r0 < R;) {
        r0 = __builtin_amdgcn_readfirstlane(r0);
        d.op = __builtin_amdgcn_readfirstlane(d.op);
        const int32_t jr = r0 + d.lane;
        LaneRec lr{uint4{0u, (uint32_t)d.op, 0u, 0u}, 0};
        if (jr < R) lr = LaneRec{d.recs[jr], d.roff[jr]};
        const uint64_t bm = __ballot(jr < R && ((int32_t)lr.rec.z > kGrpLit || (int32_t)lr.rec.w > kGrpMatch));
        const int g = bm ? (int)__builtin_ctzll(bm) : (R - r0 < 64 ? R - r0 : 64);
        if (g > 0) run_group(d, lr, g);
        if (bm) run_long(d, lr, g);
        r0 += g + (bm ? 1 : 0);
        if (d.op - d.fl >= kFlush) d.flush(d.op);
    }
}

__global__ __launch_bounds__(64) void k_decode_blocks(const uint8_t *src, int64_t src_bytes, const IngestBlock *tab,
                                                      int64_t nblocks, uint8_t *dst, int *status) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    __shared__ __attribute__((aligned(16))) uint32_t cinw[kCinWords];
    __shared__ __attribute__((aligned(16))) uint4 recs[kMaxRec];
    __shared__ uint16_t roff[kMaxRec];
    Decoder d;
    d.ring = ring, d.cinw = cinw, d.cin = reinterpret_cast<const uint8_t *>(cinw), d.recs = recs, d.roff = roff;
    d.src_end = src + src_bytes, d.lane = threadIdx.x;
    for (int64_t bi = blockIdx.x; bi < nblocks; bi += gridDim.x) {
        const IngestBlock blk = tab[bi];
        if (blk.method == 0x02) {  // stored block: one literal run (the ring copy is unused)
            copy_literals(src + blk.src, d.src_end, dst + blk.dst, 0, blk.usize, ring, d.lane);
            continue;
        }
        // (a block too large for 32-bit positions: an empty stream, which no path decodes)
        bool bad = blk.csize >= (1u << 30) || blk.usize >= (1u << 30), done = false;
        d.begin(src + blk.src, dst + blk.dst, bad ? 0 : (int32_t)blk.csize, bad ? 0 : (int32_t)blk.usize);
        if ((int64_t)d.isz * 8 >= (int64_t)d.osz * 7) {
            done = decode_by_token(d);
        } else {
            int32_t E = 0, ncs = 0;  // the next true token position (uniform); the next chunk
            for (int32_t cs = 0; cs < d.isz && !bad && !done; cs = ncs) {
                E = __builtin_amdgcn_readfirstlane(E);
                d.op = __builtin_amdgcn_readfirstlane(d.op);
                d.fl = __builtin_amdgcn_readfirstlane(d.fl);
                ncs = cs + kChunk;
                if (E >= cs + kChunk) continue;  // inside a long literal run
                stage_chunk(d, cs);
                const SpecParse a = parse_speculative(d, cs, E);
                const Chain ch = walk_chain(d, a, cs, E);
                bad = ch.bad || ch.R > kMaxRec || !write_records(d, cs, ch);
                if (bad) break;
                done = E >= d.isz;
                // the next chunk holding a token start
                ncs = E - E % kChunk > cs ? E - E % kChunk : cs + kChunk;
                __builtin_amdgcn_wave_barrier();
                // the stream ends with the literals-only sequence, the only
                // record without a match: one that ends in a match is malformed,
                // as in the token path and the reference
                bad = done && (ch.R == 0 || recs[ch.R - 1].w != 0);
                if (!bad) run_records(d, ch.R);
            }
        }
        bad = bad || !done || d.op != d.osz;
        __builtin_amdgcn_wave_barrier();
        if (!bad) d.flush(d.op);
        if (bad && d.lane == 0) atomicOr(status, 4);
        __syncthreads();
    }
}

void launch_decode_blocks(const uint8_t *src, int64_t src_bytes, const IngestBlock *tab, int64_t nblocks, uint8_t *dst,
                          int *status, hipStream_t s) {
    if (nblocks <= 0) return;
    const int grid = (int)std::min<int64_t>(nblocks, 4096);
    hipLaunchKernelGGL(k_decode_blocks, dim3(grid), dim3(64), 0, s, src, src_bytes, tab, nblocks, dst, status);
}

}  // namespace mqvs
