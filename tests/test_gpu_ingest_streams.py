"""k_decode_blocks against hand-assembled LZ4 token streams
(tests/lz4_streams.py): each test ingests one packed column, one case per
block, and compares the decoded rows bit for bit with the assembler's own
expected bytes.  The streams' bytes are arbitrary float bits, so the segments
are never searched.  tests/test_lz4_streams.py checks, on the CPU, that every
stream decodes to those bytes through the oracle and still sits on the edge
it was built for.

Malformed streams must be refused with ILLEGAL_COLUMN and leave the process
able to ingest.  The guard each one relies on: a function of csrc/lz4_token.h,
which both parse paths go through, or a decoder stage (kernels_lz4.hip) --
every one of them is checked before any record of the chunk (any copy of the
sequence) runs, and every store lies below the validated output position:
  off0, off_before_start   lz4_fits `off == 0 || off > o + ll`
  ll_past_output           lz4_fits `ll > osz - o`
  ml_past_output           lz4_fits `ml > osz - o - ll`
  lit_past_stream          lz4_parse `ll > isz - q`
  llext_to_end, mlext_to_end  lz4_extend `q >= isz`
  half_offset              lz4_parse `isz - q < 2`
  usize_plus1              k_decode_blocks, the final `op != osz`
  usize_minus1             lz4_fits `ll > osz - o` at the last literals
  ends_in_match            k_decode_blocks, `done` needs the literals-only sequence
  trailing1, trailing3     lz4_parse `isz - q < 2`; lz4_fits `ml > osz - o - ll`
"""
import ctypes

import numpy as np
import pytest

import lz4_streams as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def device_rows(seg):
    out = np.empty((seg.n, seg.d), np.float32)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipDeviceSynchronize()
    rc = hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(seg.device_rows_ptr()),
                       ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0
    return out


def ingest_and_compare(mq, col, names):
    seg = mq.VectorScanSegment.from_column(col.data, col.sizes, col.n, col.d, metric="L2")
    try:
        got = device_rows(seg).tobytes()
    finally:
        seg.free()
    mm = L.first_mismatch(col, got)
    if mm is not None:
        bi, at, g, w = mm
        wrong = L.wrong_blocks(col, got)
        pytest.fail(f"block {bi} ({names[bi] if bi < len(names) else 'pad'}): byte {at} is {g:#x}, expected {w:#x}; "
                    f"{len(wrong)} blocks with a wrong byte: {[names[i] if i < len(names) else 'pad' for i in wrong][:40]}")


@pytest.mark.parametrize("name", ["valid", "fuzz", "long"])
def test_gpu_ingest_streams(mq, name):
    """valid: offsets, near/far, far inside a group, lengths, groups and
    records, chunk and look-ahead boundaries, segment entries, in both
    regimes; fuzz: 100 seeded streams; long: length-extension runs longer
    than the look-ahead and the two constant 1 MiB blocks."""
    col, names = L.named_column(name)
    ingest_and_compare(mq, col, names)


def _small_valid():
    c = next(c for c in L.valid_cases() if c.name == "lengths/chunked")
    return L.column([c.stream]), [c.name]


@pytest.mark.parametrize("bad", L.malformed_cases() + L.trailing_cases(), ids=lambda b: b.name)
def test_gpu_ingest_malformed_stream(mq, bad):
    """trailing*: bytes after the final literals, which the reference and the
    oracle accept (they stop when the output is full); the decoder takes the
    sequence whose literals end the stream for the last one and refuses
    (DESIGN.md 3.10)."""
    from myscaledb_amd import _lib
    col = L.bad_column(bad)
    with pytest.raises(_lib.MqvsError) as e:
        mq.VectorScanSegment.from_column(col.data, col.sizes, col.n, col.d, metric="L2")
    assert e.value.status == _lib.ERR_ILLEGAL_COLUMN, str(e.value)
    assert "malformed LZ4 block" in str(e.value)
    ingest_and_compare(mq, *_small_valid())  # the process still ingests


def _ragged(n, d, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 4, n).astype(np.uint64)
    data = rng.integers(-1000, 1000, int(sizes.sum())).astype(np.float32)
    return sizes, data


@pytest.mark.parametrize("n", [4095, 4096, 4097, 4096 * 1024 + 4097])
def test_gpu_ingest_sizes_scan(mq, n):
    """The sizes scan at its tile edges (4096 sizes per tile) and above 1024
    tiles, where k_sizes_top takes more than one tile per thread: rows bit
    for bit against the oracle's copy loop, the nonempty flags through a
    filtered search that selects more rows than it can return."""
    d = 2
    sizes, data = _ragged(n, d, 17 + n % 7)
    db = O.compress_stream(data.tobytes(), 1 << 20, 0x02)
    sb = O.compress_stream(sizes.tobytes(), 1 << 20, 0x02)
    rows, ne = O.array_rows(data, sizes, d)
    seg = mq.VectorScanSegment.from_column(db, sb, n, d, metric="L2", granule=8192)
    try:
        got = device_rows(seg)
        diff = np.nonzero((got.view(np.uint32) != rows.view(np.uint32)).any(axis=1))[0]
        assert diff.size == 0, f"{diff.size} rows differ, the first at {int(diff[0])}"
        pick = np.zeros(n, bool)
        pick[np.r_[0:20, n // 2:n // 2 + 20, n - 20:n]] = True
        f = np.packbits(pick, bitorder="little")
        q = np.array([[0.25, -1.5]], np.float32)
        ids, dist = seg.search(q, 60, filter_bitmap=f)
        ids_o, dist_o = O.vector_scan(rows, q, 60, O.L2, 8192, nonempty=ne, filter_bits=f)
        assert 0 < int(ne[pick].sum()) < 60
        assert np.array_equal(ids, ids_o) and np.array_equal(dist.view(np.uint32), dist_o.view(np.uint32))
    finally:
        seg.free()


def test_gpu_ingest_oversized_sizes(mq):
    """Two sizes of 2^63 sum, modulo 2^64, to the element count of an empty
    data stream: a size above the data stream's element count is refused."""
    from myscaledb_amd import _lib
    sb = O.compress_stream(np.array([1 << 63, 1 << 63], np.uint64).tobytes())
    with pytest.raises(_lib.MqvsError) as e:
        mq.VectorScanSegment.from_column(b"", sb, 2, 4, metric="L2")
    assert e.value.status == _lib.ERR_ILLEGAL_COLUMN, str(e.value)
    assert "exceed" in str(e.value)
    ingest_and_compare(mq, *_small_valid())
