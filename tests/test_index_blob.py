"""mqvs_index_blob_info: the header of a saved index read on the host (no
device call, so these run without a GPU).  Blobs are framed by the oracle's
CompressedWriteBuffer restatement."""
import numpy as np
import pytest

from index_blob_format import KIND_BINARY, KIND_FLOAT, MAGIC, pack_header
from oracle import oracle as O


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    return m


def framed(header, body_bytes, method=0x02):
    return O.compress_stream(header + b"\0" * body_bytes, method=method)


def status_of(mq, blob):
    with pytest.raises(mq._lib.MqvsError) as e:
        mq.index_blob_info(blob)
    return e.value.status


def test_blob_info_returns_the_header_fields(mq):
    n, d, nlist = 5000, 100, 37
    hdr = pack_header(KIND_FLOAT, mq._lib.METRIC_COSINE, d, n, nlist, alpha=2.5, np95=6, fingerprint=0x0123456789ABCDEF)
    info = mq.index_blob_info(framed(hdr, 4 * nlist * d + 4 * n))
    assert info == dict(version=1, kind=KIND_FLOAT, metric=mq._lib.METRIC_COSINE, dim=d, n=n, nlist=nlist, alpha=2.5,
                        np95=6, fingerprint=0x0123456789ABCDEF, content_bytes=64 + 4 * nlist * d + 4 * n)
    n, bits, nlist = 3000, 136, 20
    hdr = pack_header(KIND_BINARY, mq._lib.METRIC_JACCARD, bits, n, nlist, fingerprint=7)
    info = mq.index_blob_info(framed(hdr, nlist * bits // 8 + 4 * n))
    assert (info["kind"], info["metric"], info["dim"], info["n"], info["nlist"], info["alpha"], info["np95"]) == \
        (KIND_BINARY, mq._lib.METRIC_JACCARD, bits, n, nlist, 3.0, 0)
    assert info["content_bytes"] == 64 + nlist * 17 + 4 * n


def test_blob_info_reads_a_first_block_smaller_than_the_content(mq):
    """A content of more than one block: the header is in the first."""
    hdr = pack_header(KIND_FLOAT, mq._lib.METRIC_L2, 64, 5000, 8)
    blob = O.compress_stream(hdr + b"\0" * (4 * 8 * 64 + 4 * 5000), block_size=4096, method=0x02)
    assert mq.index_blob_info(blob)["n"] == 5000


def test_blob_info_bad_magic(mq):
    hdr = pack_header(KIND_FLOAT, mq._lib.METRIC_L2, 64, 5000, 8, magic=b"MQVSIDY\0")
    assert status_of(mq, framed(hdr, 100)) == mq._lib.ERR_ILLEGAL_COLUMN


def test_blob_info_short_blob(mq):
    good = framed(pack_header(KIND_FLOAT, mq._lib.METRIC_L2, 64, 5000, 8), 0)
    assert len(good) == 25 + 64 and MAGIC in good
    assert mq.index_blob_info(good)["nlist"] == 8
    for cut in (0, 10, 25, 25 + 63):
        assert status_of(mq, good[:cut]) == mq._lib.ERR_ILLEGAL_COLUMN, cut
    # a first block that claims more bytes than the blob holds
    assert status_of(mq, framed(pack_header(KIND_FLOAT, mq._lib.METRIC_L2, 64, 5000, 8), 100)[:-1]) == \
        mq._lib.ERR_ILLEGAL_COLUMN


def test_blob_info_unknown_version(mq):
    hdr = pack_header(KIND_FLOAT, mq._lib.METRIC_L2, 64, 5000, 8, version=2)
    assert status_of(mq, framed(hdr, 100)) == mq._lib.ERR_NOT_IMPLEMENTED


def test_blob_info_lz4_first_block(mq):
    hdr = pack_header(KIND_FLOAT, mq._lib.METRIC_L2, 64, 5000, 8)
    blob = framed(hdr, 4 * 8 * 64 + 4 * 5000, method=0x82)
    assert blob[16] == 0x82
    assert status_of(mq, blob) == mq._lib.ERR_NOT_IMPLEMENTED
    assert np.frombuffer(O.decompress_stream(blob, 1 << 20), np.uint8)[:8].tobytes() == MAGIC
