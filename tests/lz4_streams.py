"""Hand-assembled LZ4 block streams with their own expected output, for the
column ingest decoder (k_decode_blocks).

`Stream` assembles a block sequence by sequence and extends the expected
output with the match semantics of the format itself (an overlapping match
replicates its prefix byte by byte); nothing here decodes and nothing calls
the oracle's LZ4.  `frame` adds the ClickHouse block header and checksum,
`column` packs framed blocks into a data stream with its sizes stream.

The named cases the GPU tests ingest are built here as well (`valid_cases`,
`fuzz_cases`, `long_run_cases`, `malformed_cases`), so that the CPU tests can
check every stream against the oracle's decoder and assert, on the stream
itself, the property each one was built for.
"""
import struct
from functools import lru_cache

import numpy as np

from oracle import oracle as O

# the decoder's constants (kernels_lz4.hip) the cases are cut to
K_CHUNK, K_LOOK, K_SEG, K_STARTS = 1024, 256, 16, 4
K_RING, K_FLUSH, K_GRP_LIT, K_GRP_MATCH, K_MAX_REC = 4096, 1024, 16, 27, 343

CHUNKED, TOKEN = "chunked", "token"


def is_chunked(isz, osz):
    """The decoder's own switch: blocks compressed below 7/8 are parsed in chunks."""
    return 8 * isz < 7 * osz


def _ext(v):
    """Length-extension bytes for the part of a length above 15: 255... then the remainder."""
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq_bytes(literals, off=None, ml=0, ll=None):
    """One sequence: token, literal-length extension, literals, offset,
    match-length extension.  off=None is the literals-only final sequence.
    `ll` overrides the declared literal length (malformed streams only)."""
    ll = len(literals) if ll is None else ll
    mcode = 0 if off is None else ml - 4
    assert mcode >= 0
    b = bytearray([(min(ll, 15) << 4) | min(mcode, 15)])
    if ll >= 15:
        b += _ext(ll - 15)
    b += literals
    if off is not None:
        b += struct.pack("<H", off)
        if mcode >= 15:
            b += _ext(mcode - 15)
    return bytes(b)


class Seq:
    """Where a sequence's parts lie in the compressed stream and its output."""
    __slots__ = ("tok", "lit", "offpos", "mlext", "end", "ll", "off", "ml", "out")

    def llext(self):
        return self.tok + 1 if self.ll >= 15 else None


class Stream:
    def __init__(self):
        self.comp = bytearray()
        self.out = bytearray()
        self.seqs = []

    def seq(self, literals, off=None, ml=0):
        literals = bytes(literals)
        q = Seq()
        q.tok, q.ll, q.off, q.ml, q.out = len(self.comp), len(literals), off, ml if off is not None else 0, len(self.out)
        q.lit = q.tok + 1 + (len(_ext(q.ll - 15)) if q.ll >= 15 else 0)
        q.offpos = q.mlext = None
        self.comp += seq_bytes(literals, off, ml)
        self.out += literals
        if off is not None:
            assert ml >= 4 and 1 <= off <= 65535 and off <= len(self.out), (off, ml, len(self.out))
            q.offpos = q.lit + q.ll
            q.mlext = q.offpos + 2 if ml - 4 >= 15 else None
            if off >= ml:
                self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
            else:
                out = self.out
                for _ in range(ml):
                    out.append(out[-off])
        q.end = len(self.comp)
        self.seqs.append(q)
        return q

    def raw(self, data):
        """Bytes straight into the compressed stream (malformed cases); no output."""
        self.comp += data
        return self

    @property
    def isz(self):
        return len(self.comp)

    @property
    def osz(self):
        return len(self.out)


def frame(compressed, usize, method=0x82):
    """16-byte CityHash128 + the 9-byte header (method, compressed size
    including the header, decompressed size) + payload."""
    body = struct.pack("<BII", method, 9 + len(compressed), usize) + bytes(compressed)
    return O.checksum_bytes(body) + body


class Column:
    pass


def column(blocks, d=8):
    """blocks: Stream (an LZ4 block), ("stored", bytes), ("raw", compressed,
    usize, expected or None), or ("framed", one framed block, expected).  Returns a Column: .data / .sizes streams, .n,
    .d, .expected bytes (None-expected raw blocks count as zeros), and .table
    of (src, dst, csize, usize, method) as k_block_table must find it."""
    parts, exp, table, pos, total = [], bytearray(), [], 0, 0

    def add(comp, usize, method, want, framed=None):
        nonlocal pos, total
        parts.append(frame(comp, usize, method) if framed is None else framed)
        table.append((pos + 25, total, len(comp), usize, method))
        pos += 25 + len(comp)
        total += usize
        exp.extend(want if want is not None else bytes(usize))

    for b in blocks:
        if isinstance(b, Stream):
            add(b.comp, len(b.out), 0x82, b.out)
        elif b[0] == "stored":
            add(b[1], len(b[1]), 0x02, b[1])
        elif b[0] == "framed":
            method, csize, usize = struct.unpack("<BII", b[1][16:25])
            assert 16 + csize == len(b[1]) and usize == len(b[2])
            add(b[1][25:], usize, method, b[2], b[1])
        else:
            add(b[1], b[2], 0x82, b[3])
    pad = -total % (4 * d)
    if pad:
        add(bytes(range(1, pad + 1)), pad, 0x02, bytes(range(1, pad + 1)))
    c = Column()
    c.data, c.expected, c.table, c.d, c.n = b"".join(parts), bytes(exp), table, d, total // (4 * d)
    c.sizes = frame(np.full(c.n, d, np.uint64).tobytes(), 8 * c.n, 0x02)
    return c


def first_mismatch(col, got):
    """None, or (block index, byte within the block, got, want) of the first differing byte."""
    got = np.frombuffer(got, np.uint8)
    want = np.frombuffer(col.expected, np.uint8)
    assert got.size == want.size
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    for bi, (_, dst, _, usize, _) in enumerate(col.table):
        if dst <= i < dst + usize:
            return bi, i - dst, int(got[i]), int(want[i])
    raise AssertionError


def wrong_blocks(col, got):
    """Indices of the blocks holding a differing byte."""
    ne = np.frombuffer(got, np.uint8) != np.frombuffer(col.expected, np.uint8)
    return [bi for bi, (_, dst, _, usize, _) in enumerate(col.table) if ne[dst:dst + usize].any()]


# ---- fillers: steer a block's ratio and place its sequences -------------------

def _small_off(s, rng):
    return int(min(s.osz, rng.choice((1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 100, 1000))))


def comp_seq(s, rng, ll=4):
    """A compressible filler sequence: ll fresh literals, an 18-byte match (ll + 3 bytes for ll + 18)."""
    lit = rng.bytes(ll)
    return s.seq(lit, _small_off(s, rng) if s.osz else ll, 18)


def lit_seq(s, rng, ll=200):
    """An incompressible filler sequence: ll fresh literals, a 4-byte match (ll + 4 bytes for ll + 4)."""
    lit = rng.bytes(ll)
    return s.seq(lit, _small_off(s, rng) if s.osz else 4, 4)


def fill_to(s, rng, target, regime=CHUNKED):
    """Filler sequences until the compressed stream is exactly `target` bytes long."""
    if regime == CHUNKED:
        assert target - s.isz >= 7
        while target - s.isz >= 14:
            comp_seq(s, rng)
        comp_seq(s, rng, target - s.isz - 3)
    else:
        assert target - s.isz >= 20
        while target - s.isz >= 224:
            lit_seq(s, rng)
        lit_seq(s, rng, target - s.isz - 4)
    assert s.isz == target


def prefill(s, rng, regime, out_min=2048, comp_to=None):
    """Filler of the regime's kind: at least out_min bytes of output, then (chunked
    only) on to a compressed length of exactly comp_to."""
    while s.osz < out_min:
        comp_seq(s, rng) if regime == CHUNKED else lit_seq(s, rng)
    if comp_to is not None and regime == CHUNKED:
        while comp_to - s.isz < 7:
            comp_to += K_CHUNK
        fill_to(s, rng, comp_to)
    return s


def finish(s, rng, regime, tail=5):
    """Post filler until the block is safely in `regime`, then the final literals."""
    def ratio_ok():
        isz, osz = s.isz + 1 + tail, s.osz + tail
        return 8 * isz < 7 * osz - 64 if regime == CHUNKED else 8 * isz >= 7 * osz + 64
    while not ratio_ok():
        comp_seq(s, rng) if regime == CHUNKED else lit_seq(s, rng)
    s.seq(rng.bytes(tail))
    assert is_chunked(s.isz, s.osz) == (regime == CHUNKED)
    return s


class Case:
    def __init__(self, name, stream, regime, **props):
        self.name, self.stream, self.regime, self.props = name, stream, regime, props


def _rng(name):
    return np.random.default_rng(list(name.encode()))


def _case(out, name, regime, core, out_min=2048, comp_to=None, **props):
    """prefill, core(s, rng) -> extra props or None, finish."""
    full = name + "/" + regime
    rng = _rng(full)
    s = Stream()
    prefill(s, rng, regime, out_min, comp_to)
    extra = core(s, rng) or {}
    finish(s, rng, regime, 5 + len(out) % 4)
    out.append(Case(full, s, regime, **props, **extra))


BOTH = (CHUNKED, TOKEN)

GROUP_OFFS = (1, 2, 3, 4, 5, 7, 8, 27, 28)
GROUP_MLS = (4, 5, 18, 19, 27)
BIG_SMALL_OFFS = (1, 2, 3, 5, 7)
BIG_MLS = (28, 255, 256, 257, 273, 1000)
NEARFAR_OFFS = (3839, 3840, 3841, 4095, 4096, 4097, 8192, 65535)
NEARFAR_MLS = (28, 256, 300, 5000)
LLS = (0, 1, 14, 15, 16, 17, 255, 256, 257, 270, 271, 15 + 255, 15 + 255 * 2)
MLS = (4, 18, 19, 27, 28, 273, 274, 15 + 4 + 255 * 2)
FAR_SWEEP = tuple(range(1300, 4201, 50))
GRP_LL = 11  # 64 sequences of GRP_LL literals and a 27-byte match: 15 bytes each, 960 in one chunk


@lru_cache(maxsize=None)
def valid_cases():
    cs = []
    # ---- offsets: every (off, ml) of a family in one block, a few literals between
    def offsets(pairs):
        def core(s, rng):
            for off, ml in pairs:
                s.seq(rng.bytes(int(rng.integers(1, 9))), off, ml)
            return {"pairs": pairs}
        return core
    for regime in BOTH:
        for off in GROUP_OFFS:
            _case(cs, f"grp_off{off}", regime, offsets([(off, ml) for ml in GROUP_MLS]))
        for off in BIG_SMALL_OFFS:
            _case(cs, f"big_off{off}", regime, offsets([(off, ml) for ml in BIG_MLS]))
        for off in NEARFAR_OFFS:
            _case(cs, f"nearfar_off{off}", regime, offsets([(off, ml) for ml in NEARFAR_MLS]), out_min=off + 512)
    # ---- far inside a group: lane `at` of a full group of 64 sweeps over far_lim
    for at in (0, 31, 63):
        for off in FAR_SWEEP:
            def core(s, rng, at=at, off=off):
                s.seq(rng.bytes(40), 9, 40)  # a long one: the group starts with the next record
                g0 = len(s.seqs)
                for lane in range(64):
                    s.seq(rng.bytes(GRP_LL), off if lane == at else int(rng.integers(1, 200)), K_GRP_MATCH)
                s.seq(rng.bytes(40), 9, 40)
                q = s.seqs[g0 + at]
                gend = s.seqs[g0 + 63].out + GRP_LL + K_GRP_MATCH
                return {"group": (g0, 64), "far": q.out + GRP_LL - off < gend - K_RING}
            for regime in BOTH:
                _case(cs, f"grpfar_lane{at}_off{off}", regime, core, out_min=4400, comp_to=2 * K_CHUNK - 45,
                      sweep=(at, off))
    # ---- lengths
    def lengths(s, rng):
        for ll in LLS:
            s.seq(rng.bytes(ll), int(rng.integers(1, 64)), 6)
        for ml in MLS:
            s.seq(rng.bytes(3), int(rng.integers(1, 64)), ml)
        for ll in (15, 16, 17, 256, 257):
            for ml in (27, 28, 273):
                s.seq(rng.bytes(ll), 3, ml)
    for regime in BOTH:
        _case(cs, "lengths", regime, lengths)
    # ---- groups and records
    for k in (63, 64, 65):
        def core(s, rng, k=k):
            s.seq(rng.bytes(40), 9, 40)
            g0 = len(s.seqs)
            for _ in range(k):
                s.seq(rng.bytes(int(rng.integers(0, 5))), int(rng.integers(1, 300)), int(rng.integers(4, 19)))
            s.seq(rng.bytes(40), 9, 40)
            return {"group": (g0, k)}
        for regime in BOTH:
            _case(cs, f"group{k}", regime, core, comp_to=K_CHUNK - 45)
    for c0 in (0, 1, 2):
        def core(s, rng, c0=c0):
            g0 = len(s.seqs)
            while s.isz < 3 * K_CHUNK:
                s.seq(b"", int(rng.integers(1, 400)), int(rng.integers(4, 19)))
            return {"tokens3": (g0, len(s.seqs) - g0), "c0": c0}
        for regime in BOTH:
            _case(cs, f"maxrec_at{c0}", regime, core, comp_to=K_CHUNK + c0)
    def chain(s, rng):
        s.seq(rng.bytes(40), 9, 40)
        g0 = len(s.seqs)
        for _ in range(64):
            s.seq(rng.bytes(1), 9, 8)  # the source is the previous match's output
        s.seq(rng.bytes(40), 9, 40)
        return {"group": (g0, 64)}
    def nodeps(s, rng):
        s.seq(rng.bytes(40), 9, 40)
        g0 = len(s.seqs)
        for _ in range(64):
            s.seq(rng.bytes(4), 1500, 8)  # every source lies before the group
        s.seq(rng.bytes(40), 9, 40)
        return {"group": (g0, 64)}
    for regime in BOTH:
        _case(cs, "chain64", regime, chain, comp_to=K_CHUNK - 45)
        _case(cs, "nodeps64", regime, nodeps, comp_to=K_CHUNK - 45)
    # ---- chunk and look-ahead boundaries (chunked path only)
    comps = {"tok": 0, "llext": 1, "lit": 2, "offlo": 22, "offhi": 23, "mlext": 24}  # ll 20, ml 40
    for bnd in (K_CHUNK, 2 * K_CHUNK):
        for cname, coff in comps.items():
            for t in range(1021, 1027):
                place = bnd - K_CHUNK + t
                def core(s, rng, place=place, coff=coff):
                    q = s.seq(rng.bytes(20), 7, 40)
                    return {"straddle": (q.tok + coff, place)}
                _case(cs, f"bnd{bnd}_{cname}_at{t}", CHUNKED, core, out_min=8, comp_to=place - coff)
    for ll in (256, 257, 300):  # a token near the chunk's end, literals past the staged bytes
        def core(s, rng, ll=ll):
            q = s.seq(rng.bytes(ll), 5, 9)
            s.seq(rng.bytes(2), 3, 5)  # the next token lies outside the staged bytes
            return {"past_look": (q.tok, q.lit + q.ll)}
        _case(cs, f"look_ll{ll}", CHUNKED, core, comp_to=K_CHUNK - 1)
        _case(cs, f"look_ll{ll}_at1020", CHUNKED, core, comp_to=K_CHUNK - 4)
    for ll in (1100, 2100, 3072 + 30):  # a literal run that skips whole chunks
        def core(s, rng, ll=ll):
            q = s.seq(rng.bytes(ll), 5, 9)
            return {"skips": (q.tok, q.lit + q.ll)}
        _case(cs, f"skip_ll{ll}", CHUNKED, core, comp_to=K_CHUNK + 500)
    # ---- segment entries: sequences of 3..19 bytes, token starts at every segment offset
    def entries(s, rng):
        g0 = len(s.seqs)
        while s.isz < 6 * K_CHUNK:
            ll = int(rng.integers(0, 16))  # sequences of 3..19 bytes
            s.seq(rng.bytes(ll), int(rng.integers(1, min(s.osz + ll, 3000) + 1)), int(rng.integers(4, 19)))
        return {"entries": (g0, len(s.seqs) - g0)}
    _case(cs, "segment_entries", CHUNKED, entries, out_min=64)
    return tuple(cs)


@lru_cache(maxsize=None)
def long_run_cases():
    """Length-extension runs longer than kLook.  (The two constant columns are
    compressed by the oracle in the tests themselves.)"""
    cs = []
    rng = _rng("long_runs")
    s = Stream()
    s.seq(rng.bytes(70000), 65535, 600000)
    s.seq(b"", 1, 70000)
    s.seq(rng.bytes(5))
    cs.append(Case("long_lit_match/chunked", s, CHUNKED))
    s = Stream()
    s.seq(rng.bytes(70000), 4, 4)
    s.seq(rng.bytes(6))
    cs.append(Case("long_lit/token", s, TOKEN))
    return tuple(cs)


@lru_cache(maxsize=None)
def constant_blocks():
    """1 MiB of one repeated Float32 and of one repeated 256-byte row, each one
    block of the oracle's compressor: one match of about 1 MiB at offset 4 / 256."""
    rng = _rng("constant")
    out = []
    for unit in (4, 256):
        raw = rng.bytes(unit) * ((1 << 20) // unit)
        out.append((f"constant{unit}", ("framed", O.compress_stream(raw, 1 << 20), raw)))
    return tuple(out)


def named_column(name):
    """The packed columns the GPU tests ingest: (Column, block names)."""
    if name == "valid":
        cases = valid_cases()
    elif name == "fuzz":
        cases = fuzz_cases()
    elif name == "long":
        cases = long_run_cases()
        extra = constant_blocks()
        return column([c.stream for c in cases] + [b for _, b in extra]), [c.name for c in cases] + [n for n, _ in extra]
    else:
        raise ValueError(name)
    return column([c.stream for c in cases]), [c.name for c in cases]


EDGE_LL = LLS
EDGE_ML = tuple(sorted(set(GROUP_MLS + BIG_MLS + NEARFAR_MLS + MLS)))
EDGE_OFF = tuple(sorted(set(GROUP_OFFS + NEARFAR_OFFS)))


@lru_cache(maxsize=None)
def fuzz_cases(count=100):
    """Seeded streams of 20..40 KiB: half of ll / ml / off from the edge lists,
    half uniform, off clipped to the output so far.  Even streams draw mostly
    matches, odd ones mostly literals, so that both regimes occur."""
    cs = []
    lit_ml = tuple(m for m in EDGE_ML if m <= 300)
    for i in range(count):
        rng = np.random.default_rng([0x4C5A34, i])
        want = int(rng.integers(20 << 10, 40 << 10))
        s = Stream()
        s.seq(rng.bytes(int(rng.integers(1, 40))), 1, 4)
        while s.osz < want:
            ll = int(rng.choice(EDGE_LL)) if rng.random() < 0.5 else int(rng.integers(0, 400 if i % 2 else 12))
            ml = int(rng.choice(lit_ml if i % 2 else EDGE_ML)) if rng.random() < 0.5 else \
                int(rng.integers(4, 12 if i % 2 else 400))
            off = int(rng.choice(EDGE_OFF)) if rng.random() < 0.5 else int(rng.integers(1, 65536))
            s.seq(rng.bytes(ll), min(off, s.osz + ll), ml)
            while i % 2 and is_chunked(s.isz + 9, s.osz + 8):  # literal filler keeps odd streams on the token path
                lit_seq(s, rng, 300)
        s.seq(rng.bytes(5 + i % 4))
        cs.append(Case(f"fuzz{i}", s, CHUNKED if is_chunked(s.isz, s.osz) else TOKEN))
    return tuple(cs)


# ---- malformed streams ----------------------------------------------------------

class Bad:
    """A block the decoder must refuse: compressed bytes and the declared usize."""
    def __init__(self, name, comp, usize, regime, pos, out):
        self.name, self.comp, self.usize, self.regime, self.pos, self.out = name, bytes(comp), usize, regime, pos, bytes(out)


def _bad_tails():
    """name -> f(s, rng) that appends the bad part and returns the declared usize."""
    def off0(s, rng):
        o = s.osz
        s.raw(seq_bytes(rng.bytes(4), 0, 8) + seq_bytes(rng.bytes(8)))
        return o + 20
    def off_before_start(s, rng):
        o = s.osz
        s.raw(seq_bytes(rng.bytes(4), o + 4 + 1, 8) + seq_bytes(rng.bytes(8)))
        return o + 20
    def ll_past_output(s, rng):
        o = s.osz
        s.raw(seq_bytes(rng.bytes(20), 3, 8) + seq_bytes(rng.bytes(8)))
        return o + 19
    def ml_past_output(s, rng):
        o = s.osz
        s.raw(seq_bytes(rng.bytes(4), 2, 12) + seq_bytes(rng.bytes(5)))
        return o + 4 + 11
    def lit_past_stream(s, rng):
        o = s.osz
        s.raw(seq_bytes(rng.bytes(10), None, 0, ll=40))
        return o + 40
    def llext_to_end(s, rng):
        o = s.osz
        s.raw(b"\xf0\xff\xff\xff")
        return o + 100
    def mlext_to_end(s, rng):
        o = s.osz
        s.raw(b"\x0f\x01\x00\xff\xff\xff")
        return o + 100
    def half_offset(s, rng):
        o = s.osz
        s.raw(b"\x40" + rng.bytes(4) + b"\x01")
        return o + 12
    def usize_plus1(s, rng):
        s.seq(rng.bytes(8))
        return s.osz + 1
    def usize_minus1(s, rng):
        s.seq(rng.bytes(8))
        return s.osz - 1
    def ends_in_match(s, rng):
        s.seq(rng.bytes(4), 3, 12)
        return s.osz
    return {f.__name__: f for f in (off0, off_before_start, ll_past_output, ml_past_output, lit_past_stream,
                                    llext_to_end, mlext_to_end, half_offset, usize_plus1, usize_minus1,
                                    ends_in_match)}


def _trailing_tails():
    """Accepted by the reference and the oracle (they stop once the output is
    full), refused by the decoder, which takes the sequence whose literals end
    the stream for the last one: bytes after the final literals."""
    def trailing1(s, rng):
        s.seq(rng.bytes(8))
        s.raw(b"\x00")
        return s.osz
    def trailing3(s, rng):
        s.seq(rng.bytes(8))
        s.raw(b"\x00\x01\x00")
        return s.osz
    return {f.__name__: f for f in (trailing1, trailing3)}


def _bad_set(tails):
    out = []
    for name, f in tails.items():
        for regime, where, comp_to in ((CHUNKED, "chunk0", None), (CHUNKED, "chunk2", 2 * K_CHUNK + 300),
                                       (TOKEN, "token", None)):
            rng = _rng(f"{name}/{where}")
            s = Stream()
            prefill(s, rng, regime, 2048, comp_to)
            pos = s.isz
            usize = f(s, rng)
            assert is_chunked(s.isz, usize) == (regime == CHUNKED), name
            out.append(Bad(f"{name}/{where}", s.comp, usize, regime, pos, s.out))
    return tuple(out)


@lru_cache(maxsize=None)
def malformed_cases():
    return _bad_set(_bad_tails())


@lru_cache(maxsize=None)
def trailing_cases():
    return _bad_set(_trailing_tails())


def bad_column(bad, d=8):
    return column([("raw", bad.comp, bad.usize, None)], d)
