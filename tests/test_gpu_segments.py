"""What the segment constructors refuse and what they account for, pinned to
the library as it stood before segment.hip was split out of mqvs.hip: the
status and the mqvs_last_error text of every refusal (the handle comes back
null), the hbm_bytes / split / plane_bytes each constructor reports, the
empty-base results of the two knn_*_raw functions, and mqvs_search against
mqvs_search_ex.  Every shape is tiny (n <= 40, d 3 or 65)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028235e38)
INT32_MAX = 2 ** 31 - 1
L2, IP, COSINE, HAMMING, JACCARD = 0, 1, 2, 4, 5
NOT_IMPLEMENTED, BAD_ARGUMENTS = 1, 4

ROWS_RANGE = "segment rows must be in [0, 2^32)"
DIM = "dimension must be positive"
DIM_BITS = "binary vector dimension must be a positive multiple of 8 bits"
FLOAT_METRIC = "Metric not implemented in brute force search for Float32 Vector"
BINARY_METRIC = "Metric not implemented in brute force search for Binary Vector"
GRANULE = "granule_rows must be positive"
ROW_OFFSET = "row_offset must be a non-negative multiple of granule_rows"
NULL_OUT = "null output handle"


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


@pytest.fixture(scope="module")
def lib(mq):
    from myscaledb_amd import _lib
    return _lib.lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


ROWS = np.ones((40, 65), np.float32)   # never read by a refused call
CODES = np.ones((40, 32), np.uint8)
STREAM = np.zeros(64, np.uint8)


def float_ctor(lib, which, n=17, d=3, metric=L2, granule=8, row_offset=0, rows=ROWS, mode=1, data=STREAM,
               data_bytes=64, sizes=STREAM, sizes_bytes=64, out=True):
    """One call of a float constructor by name; returns (status, handle value)."""
    h = ctypes.c_void_p(1)
    o = ctypes.byref(h) if out else None
    if which == "create":
        rc = lib.mqvs_segment_create(ptr(rows), n, d, metric, granule, None, row_offset, o)
    elif which == "create_device":
        rc = lib.mqvs_segment_create_device(ptr(rows), n, d, metric, granule, None, row_offset, o)
    elif which == "generate":
        rc = lib.mqvs_segment_generate(7, mode, n, d, metric, granule, row_offset, o)
    else:
        rc = lib.mqvs_segment_create_from_column(ptr(data), data_bytes, ptr(sizes), sizes_bytes, n, d, metric, granule,
                                                 row_offset, 0, o)
    return rc, h.value


def binary_ctor(lib, n=17, dim_bits=256, metric=HAMMING, granule=8, row_offset=0, codes=CODES, out=True):
    h = ctypes.c_void_p(1)
    rc = lib.mqvs_segment_create_binary(ptr(codes), n, dim_bits, metric, granule, row_offset, 0,
                                        ctypes.byref(h) if out else None)
    return rc, h.value


def refused(lib, got, status, text):
    rc, handle = got
    assert rc == status
    assert lib.mqvs_last_error().decode() == text
    assert handle is None


FLOAT_CTORS = ["create", "create_device", "generate", "from_column"]

# the checks every float constructor shares, in the order the library makes them
FLOAT_REFUSALS = [
    (dict(n=-1), BAD_ARGUMENTS, ROWS_RANGE),
    (dict(n=2 ** 32), BAD_ARGUMENTS, ROWS_RANGE),
    (dict(d=0), BAD_ARGUMENTS, DIM),
    (dict(metric=HAMMING), NOT_IMPLEMENTED, FLOAT_METRIC),
    (dict(granule=0), BAD_ARGUMENTS, GRANULE),
    (dict(row_offset=-8), BAD_ARGUMENTS, ROW_OFFSET),
    (dict(row_offset=5), BAD_ARGUMENTS, ROW_OFFSET),
    # two faults: the earlier check speaks
    (dict(n=-1, d=0), BAD_ARGUMENTS, ROWS_RANGE),
    (dict(d=0, metric=JACCARD), BAD_ARGUMENTS, DIM),
    (dict(metric=HAMMING, granule=0), NOT_IMPLEMENTED, FLOAT_METRIC),
    (dict(granule=0, row_offset=-8), BAD_ARGUMENTS, GRANULE),
]


@pytest.mark.parametrize("which", FLOAT_CTORS)
def test_float_constructor_refusals(lib, which):
    for kw, status, text in FLOAT_REFUSALS:
        refused(lib, float_ctor(lib, which, **kw), status, text)
    rc, handle = float_ctor(lib, which, out=False)
    assert rc == BAD_ARGUMENTS and lib.mqvs_last_error().decode() == NULL_OUT
    # a null handle is seen before any other fault
    rc, handle = float_ctor(lib, which, n=-1, out=False)
    assert rc == BAD_ARGUMENTS and lib.mqvs_last_error().decode() == NULL_OUT


@pytest.mark.parametrize("which", ["create", "create_device"])
def test_null_rows_refused(lib, which):
    refused(lib, float_ctor(lib, which, rows=None), BAD_ARGUMENTS, "null rows")
    # the shape is checked first
    refused(lib, float_ctor(lib, which, rows=None, granule=0), BAD_ARGUMENTS, GRANULE)
    refused(lib, float_ctor(lib, which, rows=None, row_offset=5), BAD_ARGUMENTS, ROW_OFFSET)


def test_generator_mode_refused(lib):
    text = "generator mode must be 0, 1, 2 or 3"
    refused(lib, float_ctor(lib, "generate", mode=4), BAD_ARGUMENTS, text)
    refused(lib, float_ctor(lib, "generate", mode=-1), BAD_ARGUMENTS, text)
    refused(lib, float_ctor(lib, "generate", mode=4, granule=0), BAD_ARGUMENTS, GRANULE)


def test_from_column_stream_refusals(lib):
    neg, null = "negative stream size", "null column stream"
    refused(lib, float_ctor(lib, "from_column", data_bytes=-1), BAD_ARGUMENTS, neg)
    refused(lib, float_ctor(lib, "from_column", sizes_bytes=-1), BAD_ARGUMENTS, neg)
    refused(lib, float_ctor(lib, "from_column", data=None), BAD_ARGUMENTS, null)
    refused(lib, float_ctor(lib, "from_column", sizes=None), BAD_ARGUMENTS, null)
    # two faults: sizes before pointers, the shape before both
    refused(lib, float_ctor(lib, "from_column", data=None, sizes_bytes=-1), BAD_ARGUMENTS, neg)
    refused(lib, float_ctor(lib, "from_column", data=None, d=0), BAD_ARGUMENTS, DIM)


def test_binary_constructor_refusals(lib):
    for kw, status, text in [
        (dict(n=-1), BAD_ARGUMENTS, ROWS_RANGE),
        (dict(n=2 ** 32), BAD_ARGUMENTS, ROWS_RANGE),
        (dict(dim_bits=0), BAD_ARGUMENTS, DIM_BITS),
        (dict(dim_bits=12), BAD_ARGUMENTS, DIM_BITS),
        (dict(metric=L2), NOT_IMPLEMENTED, BINARY_METRIC),
        (dict(granule=0), BAD_ARGUMENTS, GRANULE),
        (dict(row_offset=-8), BAD_ARGUMENTS, ROW_OFFSET),
        (dict(row_offset=5), BAD_ARGUMENTS, ROW_OFFSET),
        (dict(codes=None), BAD_ARGUMENTS, "null codes"),
        # two faults: the shape is checked before the codes pointer
        (dict(codes=None, granule=0), BAD_ARGUMENTS, GRANULE),
        (dict(codes=None, metric=COSINE), NOT_IMPLEMENTED, BINARY_METRIC),
        (dict(n=-1, dim_bits=12), BAD_ARGUMENTS, ROWS_RANGE),
        (dict(dim_bits=12, metric=L2), BAD_ARGUMENTS, DIM_BITS),
    ]:
        refused(lib, binary_ctor(lib, **kw), status, text)
    rc, handle = binary_ctor(lib, out=False)
    assert rc == BAD_ARGUMENTS and lib.mqvs_last_error().decode() == NULL_OUT
    rc, handle = binary_ctor(lib, dim_bits=12, out=False)
    assert rc == BAD_ARGUMENTS and lib.mqvs_last_error().decode() == NULL_OUT


# ---------------------------------------------------------------------------
# accounting

GRAN = 8


def expect_bytes(n, d, bitmap, planes):
    dpad = (d + 63) // 64 * 64
    plane = 2 * ((max(n, 1) + 15) // 16 * 16) * dpad if planes else 0
    total = 4 * max(n, 1) * d + 4 * n + plane
    if bitmap:
        total += (n + 7) // 8 + 4 * ((n + GRAN - 1) // GRAN)
    return total, plane


def check_info(seg, n, d, metric, bitmap, planes):
    try:
        info = seg.info()
    finally:
        seg.free()
    total, plane = expect_bytes(n, d, bitmap, planes)
    assert (info["n"], info["d"], info["metric"], info["granule"], info["row_offset"]) == (n, d, metric, GRAN, 0)
    assert info["hbm_bytes"] == total
    assert info["prefilter"] == (2 if planes else 0)
    assert info["plane_bytes"] == plane


@pytest.fixture(params=[True, False], ids=["planes", "noplanes"])
def planes(mq, request):
    from myscaledb_amd import vector_scan
    vector_scan.set_prefilter(2 if request.param else 0)
    yield request.param
    vector_scan.set_prefilter(2)


def some_zero(n):
    ne = np.ones(n, np.uint8)
    ne[::3] = 0
    return ne


@pytest.mark.parametrize("metric", [L2, COSINE])
@pytest.mark.parametrize("d", [3, 65])
@pytest.mark.parametrize("n", [0, 1, 17, 40])
def test_float_segment_bytes(mq, planes, n, d, metric):
    import torch
    rows = O.generate(5, 1, 0, max(n, 1), d)[:n]
    VS = mq.VectorScanSegment
    # host rows: a bitmap only when some array is empty
    for ne, bitmap in ((None, False), (np.ones(n, np.uint8), False), (some_zero(n), n > 0)):
        check_info(VS.from_rows(rows, metric=metric, granule=GRAN, nonempty=ne), n, d, metric, bitmap, planes)
    check_info(VS.generate(9, 1, n, d, metric=metric, granule=GRAN), n, d, metric, False, planes)
    if n == 0:
        return
    # device rows: the flags, when given, are packed as they are
    drows = torch.from_numpy(rows).cuda()
    check_info(VS.from_rows(drows, metric=metric, granule=GRAN), n, d, metric, False, planes)
    dne = torch.from_numpy(some_zero(n)).cuda()
    check_info(VS.from_rows(drows, metric=metric, granule=GRAN, nonempty=dne), n, d, metric, True, planes)
    # column files: whole arrays decode straight into the rows (no bitmap);
    # a ragged column goes through the copy loop, which writes the flags
    ragged = np.where(some_zero(n), d, 0).astype(np.uint64)
    ragged[0] = d - 1
    for sizes, bitmap in ((np.full(n, d, np.uint64), False), (ragged, True)):
        data = np.random.default_rng(6).standard_normal(int(sizes.sum())).astype(np.float32)
        db = O.compress_stream(data.tobytes(), 1 << 20, 0x82)
        sb = O.compress_stream(sizes.tobytes(), 1 << 20, 0x82)
        for verify in (True, False):
            check_info(VS.from_column(db, sb, n, d, metric=metric, granule=GRAN, verify_checksum=verify), n, d, metric,
                       bitmap, planes)


@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
@pytest.mark.parametrize("dim_bits,words", [(8, 4), (136, 8), (256, 8)])
@pytest.mark.parametrize("n", [0, 1, 17, 40])
def test_binary_segment_bytes(mq, lib, n, dim_bits, words, metric):
    codes = np.random.default_rng(3).integers(0, 256, (n, dim_bits // 8), dtype=np.uint8)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric, granule=GRAN)
    try:
        nn, d, m, g, o = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        b, pb = ctypes.c_size_t(), ctypes.c_size_t(1)
        sp, ok = ctypes.c_int32(1), ctypes.c_int32(1)
        assert lib.mqvs_segment_info(seg._h, ctypes.byref(nn), ctypes.byref(d), ctypes.byref(m), ctypes.byref(g),
                                     ctypes.byref(o), ctypes.byref(b)) == 0
        assert lib.mqvs_segment_prefilter(seg._h, ctypes.byref(sp), ctypes.byref(pb), ctypes.byref(ok)) == 0
    finally:
        seg.free()
    assert (nn.value, d.value, m.value, g.value, o.value) == (n, dim_bits, metric, GRAN, 0)
    assert b.value == max(n, 1) * words * 4
    assert (sp.value, pb.value, ok.value) == (0, 0, 0)


# ---------------------------------------------------------------------------
# empty base

@pytest.mark.parametrize("metric,fill", [(L2, FLT_MAX), (IP, -FLT_MAX)])
def test_knn_raw_empty_base(mq, metric, fill):
    nx, k, d = 3, 4, 3
    x = O.generate(1, 1, 0, nx, d)
    ids, dist = mq.try_brute_force_search(x, np.empty((0, d), np.float32), d, k, nx, 0, metric)
    assert np.array_equal(ids, np.full(nx * k, -1, np.int64))
    assert np.array_equal(dist.view(np.uint32), np.full(nx * k, fill, np.float32).view(np.uint32))


@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
def test_knn_binary_raw_empty_base(mq, metric):
    nx, k, d = 3, 4, 136
    x = np.random.default_rng(1).integers(0, 256, (nx, d // 8), dtype=np.uint8)
    ids, dist = mq.try_brute_force_search_binary(x, np.empty((0, d // 8), np.uint8), d, k, nx, 0, metric)
    assert np.array_equal(ids, np.full(nx * k, -1, np.int64))
    if metric == HAMMING:
        assert dist.dtype == np.int32 and np.array_equal(dist, np.full(nx * k, INT32_MAX, np.int32))
    else:
        assert np.array_equal(dist.view(np.uint32), np.full(nx * k, FLT_MAX, np.float32).view(np.uint32))


@pytest.mark.parametrize("nx,k", [(0, 4), (3, 0)])
@pytest.mark.parametrize("ny", [0, 17])
def test_knn_raw_nothing_to_do_touches_nothing(lib, nx, k, ny):
    d = 8  # 8 floats, or one byte of bits
    ids = np.full(12, 77, np.int64)
    dist = np.full(12, 5.5, np.float32)
    x, y = np.ones((3, d), np.float32), np.ones((17, d), np.float32)
    for metric in (L2, IP):
        assert lib.mqvs_knn_raw(ptr(x), ptr(y), d, k, nx, ny, metric, ptr(ids), ptr(dist)) == 0
    xb, yb = np.ones((3, 1), np.uint8), np.ones((17, 1), np.uint8)
    for metric in (HAMMING, JACCARD):
        assert lib.mqvs_knn_binary_raw(ptr(xb), ptr(yb), d, k, nx, ny, metric, ptr(ids), ptr(dist)) == 0
    assert np.all(ids == 77) and np.all(dist == np.float32(5.5))


# ---------------------------------------------------------------------------
# mqvs_search_ex

def test_search_ex_base(mq, lib):
    n, d, nq, k = 40, 3, 5, 10
    rows = O.generate(11, 1, 0, n, d)
    q = O.generate(12, 1, 0, nq, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="Cosine", granule=GRAN)
    try:
        out = []
        for base in (None, -1, INT32_MAX + 1):
            ids = np.full((nq, k), 77, np.int64)
            dist = np.full((nq, k), 5.5, np.float32)
            if base is None:
                rc = lib.mqvs_search(seg._h, ptr(q), nq, k, COSINE, None, None, ptr(ids), ptr(dist), 0, None)
            else:
                rc = lib.mqvs_search_ex(seg._h, ptr(q), nq, k, COSINE, None, None, base, ptr(ids), ptr(dist), 0, None)
            out.append((rc, ids, dist))
            if base == INT32_MAX + 1:
                assert rc == BAD_ARGUMENTS and lib.mqvs_last_error().decode() == "chunk_ord_base out of range"
                assert np.all(ids == 77) and np.all(dist == np.float32(5.5))
        ids_o, dist_o = O.vector_scan(rows, q, k, O.COSINE, GRAN)
    finally:
        seg.free()
    (rc0, ids0, dist0), (rc1, ids1, dist1) = out[:2]
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(ids0, ids1) and np.array_equal(dist0.view(np.uint32), dist1.view(np.uint32))
    assert np.array_equal(ids0, ids_o) and np.array_equal(dist0.view(np.uint32), dist_o.view(np.uint32))
