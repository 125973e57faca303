"""The hand-assembled LZ4 streams of tests/lz4_streams.py, on the CPU: every
valid stream the GPU tests ingest decodes through the oracle to the
assembler's own expected bytes, and every stream still has the property it
was built for (its regime, the byte that straddles a chunk boundary, the
tokens of a group in one chunk, ...), so that an edit to a generator cannot
silently move a case off its edge."""
import struct

import numpy as np
import pytest

import lz4_streams as L
from oracle import oracle as O


def _decode(comp, usize):
    return O.decompress_stream(L.frame(comp, usize), usize)


def test_assembler_bytes():
    s = L.Stream()
    s.seq(b"abcd", 4, 4)
    s.seq(b"wxyz")
    assert bytes(s.comp) == bytes([0x40]) + b"abcd" + struct.pack("<H", 4) + bytes([0x40]) + b"wxyz"
    assert bytes(s.out) == b"abcdabcdwxyz"
    s = L.Stream()
    s.seq(b"ab", 1, 5)  # an overlapping match replicates its prefix
    s.seq(b"c", 3, 7)
    assert bytes(s.out) == b"abbbbbb" + b"c" + b"bbcbbcb"
    # length extensions: 255... then the remainder, a zero byte when the length is 15 + 255 j
    assert L.seq_bytes(b"x" * 15, 1, 4) == b"\xf0\x00" + b"x" * 15 + b"\x01\x00"
    assert L.seq_bytes(b"x" * 270, 1, 4)[:3] == b"\xf0\xff\x00"
    assert L.seq_bytes(b"", 2, 19) == b"\x0f\x02\x00\x00"
    assert L.seq_bytes(b"", 2, 18) == b"\x0e\x02\x00"
    assert L.seq_bytes(b"", 2, 4 + 15 + 255 * 2 + 1) == b"\x0f\x02\x00\xff\xff\x01"
    q = L.Stream().seq(b"y" * 20, 7, 40)
    assert (q.tok, q.llext(), q.lit, q.offpos, q.mlext, q.end) == (0, 1, 2, 22, 24, 25)


def test_frame_and_column():
    s = L.Stream()
    s.seq(b"abcd", 4, 4)
    s.seq(b"wxyz!")
    col = L.column([s, ("stored", b"0123456")])
    assert len(col.expected) == col.n * col.d * 4 and col.n == 1
    assert col.expected[:20] == b"abcdabcdwxyz!0123456"
    assert [t[3] for t in col.table] == [13, 7, 12] and col.table[-1][4] == 0x02  # the pad block
    assert O.decompress_stream(col.data, len(col.expected)) == col.expected
    assert O.decompress_stream(col.sizes, 8 * col.n) == np.full(col.n, col.d, np.uint64).tobytes()
    for src, _, csize, usize, method in col.table:
        assert struct.unpack("<BII", col.data[src - 9:src]) == (method, csize + 9, usize)


ALL_VALID = L.valid_cases() + L.long_run_cases() + L.fuzz_cases()


def test_valid_streams_decode_to_expected():
    """Block by block, so that a disagreement names its case."""
    for c in ALL_VALID:
        s = c.stream
        assert _decode(s.comp, s.osz) == bytes(s.out), c.name
        assert L.is_chunked(s.isz, s.osz) == (c.regime == L.CHUNKED), c.name


@pytest.mark.parametrize("name", ["valid", "fuzz", "long"])
def test_columns(name):
    col, names = L.named_column(name)
    assert O.decompress_stream(col.data, len(col.expected)) == col.expected
    assert len(names) in (len(col.table), len(col.table) - 1)
    if name == "long":
        # the two constant blocks are one long match each
        for (_, _, csize, usize, _), nm in zip(col.table, names):
            if nm.startswith("constant"):
                assert usize == 1 << 20 and csize < 6000, (nm, csize)
    if name == "valid":
        lz4 = [t for t in col.table if t[4] == 0x82]
        assert {t[0] & 3 for t in lz4} == {0, 1, 2, 3}
        assert {t[1] & 3 for t in lz4} == {0, 1, 2, 3}
        assert any(t[3] & 3 for t in lz4)


def test_required_combinations_present():
    names = {c.name for c in L.valid_cases()}
    for regime in L.BOTH:
        for off in L.GROUP_OFFS:
            assert f"grp_off{off}/{regime}" in names
        for off in L.BIG_SMALL_OFFS:
            assert f"big_off{off}/{regime}" in names
        for off in L.NEARFAR_OFFS:
            assert f"nearfar_off{off}/{regime}" in names
    by = {c.name: c for c in L.valid_cases()}
    for c in by.values():
        if "pairs" in c.props:  # the pairs are in the stream as stated
            have = {(q.off, q.ml) for q in c.stream.seqs}
            assert set(c.props["pairs"]) <= have, c.name
    assert (3841, 5000) in by["nearfar_off3841/chunked"].props["pairs"]
    grp = {p for c in by.values() if c.name.startswith("grp_off") for p in c.props["pairs"]}
    big = {p for c in by.values() if c.name.startswith("big_off") for p in c.props["pairs"]}
    assert {(3, 4), (3, 5), (4, 5), (5, 5)} <= grp and {(o, m) for o in L.BIG_SMALL_OFFS for m in (257, 273, 1000)} <= big
    assert all(m <= L.K_GRP_MATCH for _, m in grp) and all(m > L.K_GRP_MATCH for _, m in big)
    lens = by["lengths/chunked"].stream.seqs
    assert set(L.LLS) <= {q.ll for q in lens} and set(L.MLS) <= {q.ml for q in lens}
    assert {15 + 255, 15 + 510} <= set(L.LLS)


def _chunk(pos):
    return pos // L.K_CHUNK


def _short(q):
    return q.ll <= L.K_GRP_LIT and q.ml <= L.K_GRP_MATCH


def test_group_cases_sit_in_one_chunk():
    seen = 0
    for c in L.valid_cases():
        if "group" not in c.props or c.regime != L.CHUNKED:
            continue
        seen += 1
        g0, k = c.props["group"]
        seqs = c.stream.seqs
        grp = seqs[g0:g0 + k]
        assert grp[0].tok % L.K_CHUNK == 0, c.name  # the first record of its chunk
        assert {_chunk(q.tok) for q in grp} == {_chunk(grp[0].tok)}, c.name
        assert all(_short(q) for q in grp) and not _short(seqs[g0 - 1]) and not _short(seqs[g0 + k]), c.name
        assert _chunk(seqs[g0 + k].tok) == _chunk(grp[0].tok), c.name
    assert seen == 3 * len(L.FAR_SWEEP) + 3 + 2


def test_far_sweep_crosses_the_ring_limit():
    """far_lim = gend - kRing: for each placement of the swept lane the sweep
    has sources on both sides of it, and the group writes close to the most a
    chunk of token starts allows."""
    for at in (0, 31, 63):
        far = [c.props["far"] for c in L.valid_cases()
               if c.regime == L.CHUNKED and c.props.get("sweep", (None,))[0] == at]
        assert len(far) == len(L.FAR_SWEEP) and far[0] is False and far[-1] is True, at
        assert far == sorted(far), at
    c = next(c for c in L.valid_cases() if c.name == "grpfar_lane0_off1300/chunked")
    g0, k = c.props["group"]
    assert c.stream.seqs[g0 + k].tok - c.stream.seqs[g0].tok == 960  # 64 more bytes would leave the chunk
    for name, dep in (("chain64/chunked", True), ("nodeps64/chunked", False)):
        c = next(c for c in L.valid_cases() if c.name == name)
        g0, k = c.props["group"]
        grp = c.stream.seqs[g0:g0 + k]
        for a, b in zip(grp, grp[1:]):
            src = b.out + b.ll - b.off
            assert (src == a.out + a.ll) == dep, name  # the previous match's output, or before the group
            assert dep or src + b.ml <= grp[0].out


def test_max_records_per_chunk():
    for c in L.valid_cases():
        if "tokens3" not in c.props or c.regime != L.CHUNKED:
            continue
        g0, k = c.props["tokens3"]
        seqs = c.stream.seqs[g0:g0 + k]
        assert all(q.end - q.tok == 3 for q in seqs)
        assert seqs[0].tok == L.K_CHUNK + c.props["c0"]
        starts = [sum(1 for q in c.stream.seqs if _chunk(q.tok) == ch) for ch in (1, 2)]
        assert starts[0] == (342 if c.props["c0"] == 0 else 341), (c.name, starts)
        assert starts[1] in (341, 342) and max(starts) <= L.K_MAX_REC
    both = {sum(1 for q in c.stream.seqs if _chunk(q.tok) == ch)
            for c in L.valid_cases() if "tokens3" in c.props and c.regime == L.CHUNKED for ch in (1, 2)}
    assert both == {341, 342}


def test_boundary_cases_straddle_where_stated():
    seen = set()
    for c in L.valid_cases():
        p = c.props
        if "straddle" in p:
            assert p["straddle"][0] == p["straddle"][1], c.name
            seen.add(p["straddle"][1])
        if "past_look" in p:
            tok, end = p["past_look"]
            assert tok in (L.K_CHUNK - 1, L.K_CHUNK - 4), c.name
            assert tok != L.K_CHUNK - 1 or end > L.K_CHUNK + L.K_LOOK, c.name
            nxt = next(q for q in c.stream.seqs if q.tok > tok)
            assert nxt.tok == end + 2  # right after the offset: outside the staged bytes
        if "skips" in p:
            tok, end = p["skips"]
            assert _chunk(tok) == 1 and _chunk(end) == 1 + (end - tok) // L.K_CHUNK, c.name
    assert seen == set(range(1021, 1027)) | set(range(2045, 2051))
    assert {_chunk(c.props["skips"][1]) for c in L.valid_cases() if "skips" in c.props} == {2, 3, 4}
    names = {c.name for c in L.valid_cases()}
    for bnd in (1024, 2048):
        for comp in ("tok", "llext", "lit", "offlo", "offhi", "mlext"):
            for t in range(1021, 1027):
                assert f"bnd{bnd}_{comp}_at{t}/chunked" in names


def test_segment_entries_cover_every_offset():
    c = next(c for c in L.valid_cases() if c.name == "segment_entries/chunked")
    g0, k = c.props["entries"]
    seqs = c.stream.seqs[g0:g0 + k]
    assert {q.end - q.tok for q in seqs} == set(range(3, 20)) - {18}  # 15 literals take an extension byte
    entry = {}
    for q in seqs:
        entry.setdefault(q.tok // L.K_SEG, q.tok % L.K_SEG)  # the first token start of each segment
    assert set(entry.values()) == set(range(L.K_SEG))
    assert sum(1 for v in entry.values() if v >= L.K_STARTS) > 50


def test_fuzz_has_both_regimes():
    cases = L.fuzz_cases()
    assert len(cases) == 100
    regimes = [c.regime for c in cases]
    assert regimes.count(L.CHUNKED) >= 30 and regimes.count(L.TOKEN) >= 30
    for c in cases:
        assert 20 << 10 <= c.stream.osz <= 48 << 10, c.name
    offs = {q.off for c in cases for q in c.stream.seqs if q.off}
    assert {1, 2, 3, 5, 7, 3840, 3841, 4096, 4097, 8192} <= offs


@pytest.mark.parametrize("bad", L.malformed_cases(), ids=lambda b: b.name)
def test_malformed_streams_are_refused_by_the_oracle(bad):
    with pytest.raises(ValueError, match="CANNOT_DECOMPRESS"):
        _decode(bad.comp, bad.usize)
    _check_placement(bad)


@pytest.mark.parametrize("bad", L.trailing_cases(), ids=lambda b: b.name)
def test_trailing_bytes_are_accepted_by_the_oracle(bad):
    """The one deliberate deviation of the GPU decoder."""
    assert _decode(bad.comp, bad.usize) == bad.out
    _check_placement(bad)


def _check_placement(bad):
    assert L.is_chunked(len(bad.comp), bad.usize) == (bad.regime == L.CHUNKED)
    where = bad.name.split("/")[1]
    if where == "chunk0":
        assert bad.pos < L.K_CHUNK and bad.pos // L.K_SEG >= 1
    elif where == "chunk2":
        assert _chunk(bad.pos) == 2
    if bad.regime == L.CHUNKED:  # after at least 2 KiB of valid compressible sequences
        assert len(bad.out) >= 2048
