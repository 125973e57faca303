"""Index persistence (mqvs_index_save / mqvs_index_load, include/mqvs.h) on the
GPU.  Nothing here has a tolerance: a loaded index is the built one -- same
info, same centroid bytes, same lists, same probes, same search bits --, the
blob parses as documented with the oracle's CompressedReadBuffer and CityHash,
and the device grouping equals numpy's stable sort on assignments no build
produces (forged blobs).  "Exhaustive" below is the index tests' setting at
which an index search equals FLAT bit for bit: nprobe = nlist, num_reorder 4096.
"""
import ctypes

import numpy as np
import pytest

from index_blob_format import (IVF_PAD, KIND_BINARY, KIND_FLOAT, MAGIC, np_lists, pack_header, parse_header,
                               split_content, with_assignment)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.40282347e+38)
K = 10


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def same(a, b, ctx):
    (ia, da), (ib, db) = a, b
    assert np.array_equal(ia, ib), ctx
    assert np.array_equal(np.asarray(da, np.float32).view(np.uint32), np.asarray(db, np.float32).view(np.uint32)), ctx


def info_without_time(idx):
    info = idx.info()
    info.pop("build_ms")
    return info


def bitmaps(n, seed):
    rng = np.random.default_rng(seed)
    flt = np.packbits((rng.random(n) < 0.4).astype(np.uint8), bitorder="little")
    ex = np.packbits((rng.random(n) >= 0.1).astype(np.uint8), bitorder="little")
    return flt, ex


def codes_of(rng, n, nbytes, density=0.5):
    return np.packbits(rng.random((n, nbytes * 8)) < density, axis=1, bitorder="little")


def clustered_codes(seed, n, nq, nbytes):
    rng = np.random.default_rng(seed)
    cen = codes_of(rng, 64, nbytes)
    rows = cen[rng.integers(64, size=n)] ^ codes_of(rng, n, nbytes, 0.10)
    queries = rows[rng.choice(n, nq, replace=False)] ^ codes_of(rng, nq, nbytes, 0.05)
    return rows, queries


def assert_same_index(mq, ld, ref, queries, nlist, n, binary, ctx):
    """Every observable of the loaded index `ld` equals the built `ref`."""
    assert info_without_time(ld) == info_without_time(ref), ctx
    assert ld.centroids().tobytes() == ref.centroids().tobytes(), ctx
    for a, b in zip(ld.lists(), ref.lists()):
        assert np.array_equal(a, b), ctx
    assert np.array_equal(np.sort(ld.probes(queries[:16]), axis=1), np.sort(ref.probes(queries[:16]), axis=1)), ctx
    flt, ex = bitmaps(n, 7)
    for nq in (5, 24):
        q = queries[:nq]
        for what, kw in (("default", {}), ("every list", dict(params={"nprobe": nlist})),
                         ("filter + deletes", dict(filter_bitmap=flt, row_exists=ex)),
                         ("first stage", dict(first_stage_only=True))):
            same(ld.search(q, K, **kw), ref.search(q, K, **kw), f"{ctx} nq {nq} {what}")


FLOAT_CASES = [(64, "L2", False), (100, "L2", False), (64, "IP", False), (100, "IP", False), (64, "Cosine", False),
               (100, "Cosine", False), (64, "L2", True)]


@pytest.mark.parametrize("d,metric,holes", FLOAT_CASES, ids=[f"d{d}_{m}{'_empty_nan' if h else ''}" for d, m, h in FLOAT_CASES])
def test_float_round_trip(mq, d, metric, holes):
    n, nlist = 5000, 37
    rows = O.generate(0x5EED0101, 2, 0, n, d)
    queries = O.generate(0x5EED0102, 2, 0, 24, d)
    nonempty = None
    if holes:  # 200 empty arrays (FLT_MAX rows, in no list) and one row holding a NaN (list 0)
        nonempty = np.ones(n, np.uint8)
        nonempty[np.random.default_rng(3).choice(n, 200, replace=False)] = 0
        rows[nonempty == 0] = FLT_MAX
        nan_row = int(np.flatnonzero(nonempty)[1234])
        rows[nan_row, 5] = np.nan
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=1024, nonempty=nonempty)
    ref = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    ld = None
    try:
        blob = idx.save()
        size = ctypes.c_size_t()
        mq._lib.check(mq._lib.lib.mqvs_index_save_size(idx._h, ctypes.byref(size)))
        assert len(blob) == size.value == 64 + 4 * nlist * d + 4 * n + 25 * -(-(64 + 4 * nlist * d + 4 * n) // (1 << 20))
        idx.free()
        ld = mq.VectorIndex.load(seg, blob)
        ctx = f"d {d} {metric}"
        assert_same_index(mq, ld, ref, queries, nlist, n, False, ctx)
        assert ld.save() == blob, "save(load(save(idx))) != save(idx)"
        if holes:
            off, lrows = ld.lists()
            assert ld.info()["rows_indexed"] == n - 200 and not np.isin(np.flatnonzero(nonempty == 0), lrows).any()
            assert nan_row in lrows[off[0]:off[1]]
        for nq in (5, 24):
            ex = {"nprobe": nlist, "num_reorder": 4096}
            same(ld.search(queries[:nq], K, ex), seg.search(queries[:nq], K), f"{ctx} nq {nq} exhaustive vs FLAT")
    finally:
        for x in (ld, idx, ref, seg):
            if x is not None:
                x.free()


BINARY_CASES = [(64, "Hamming"), (136, "Hamming"), (64, "Jaccard"), (136, "Jaccard")]


@pytest.mark.parametrize("bits,metric", BINARY_CASES, ids=[f"b{b}_{m}" for b, m in BINARY_CASES])
def test_binary_round_trip(mq, bits, metric):
    n, nlist, nbytes = 3000, 20, bits // 8
    codes, queries = clustered_codes(11, n, 24, nbytes)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric, granule=1024)
    ref = mq.BinaryVectorIndex.build(seg, "BINARYMSTG", {"nlist": nlist})
    idx = mq.BinaryVectorIndex.build(seg, "BINARYMSTG", {"nlist": nlist})
    ld = None
    try:
        blob = idx.save()
        size = ctypes.c_size_t()
        mq._lib.check(mq._lib.lib.mqvs_index_save_size(idx._h, ctypes.byref(size)))
        assert len(blob) == size.value == 64 + nlist * nbytes + 4 * n + 25
        idx.free()
        ld = mq.BinaryVectorIndex.load(seg, blob)
        ctx = f"{bits} bits {metric}"
        assert_same_index(mq, ld, ref, queries, nlist, n, True, ctx)
        assert ld.save() == blob, "save(load(save(idx))) != save(idx)"
        for nq in (5, 24):
            same(ld.search(queries[:nq], K, {"nprobe": nlist}), seg.search(queries[:nq], K),
                 f"{ctx} nq {nq} every list vs part search")
    finally:
        for x in (ld, idx, ref, seg):
            if x is not None:
                x.free()


# ---- side properties ---------------------------------------------------------

def test_row_offset_segment_returns_offset_ids(mq):
    n, d, nlist, gran = 5000, 64, 8, 512
    rows = O.generate(0x5EED0101, 2, 0, n, d)
    q = O.generate(0x5EED0102, 2, 0, 5, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=gran, row_offset=2 * gran)
    ref = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    ld = mq.VectorIndex.load(seg, ref.save())
    try:
        ids, dist = ld.search(q, K)
        assert ids.min() >= 2 * gran
        same((ids, dist), ref.search(q, K), "row_offset")
        same(ld.search(q, K, {"nprobe": nlist, "num_reorder": 4096}), seg.search(q, K), "row_offset exhaustive")
        # the row-ids map of a decoupled part is not in the blob: registered again, it maps the same ids
        row_ids_map = np.random.default_rng(9).permutation(2 * gran + n).astype(np.uint64)
        ld.set_row_ids_map(row_ids_map)
        mapped = ld.search(q, K)
        assert np.array_equal(mapped[0], row_ids_map[ids].astype(np.int64))
        ref.set_row_ids_map(row_ids_map)
        same(mapped, ref.search(q, K), "row_ids_map")
    finally:
        ld.free()
        ref.free()
        seg.free()


def test_load_on_host_rows_gives_the_same_bits(mq):
    """The rows moved to host memory before the load: the fingerprint and the
    plane pack read them through the mapped address."""
    n, d, nlist = 5000, 100, 37
    rows = O.generate(0x5EED0101, 2, 0, n, d)
    q = O.generate(0x5EED0102, 2, 0, 24, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="Cosine", granule=1024)
    ref = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    blob = ref.save()
    expect = [ref.search(q[:nq], K) for nq in (5, 24)]
    info, lists = info_without_time(ref), ref.lists()
    ref.free()
    seg.set_rows_host(True)
    ld = mq.VectorIndex.load(seg, blob)
    try:
        assert seg.info()["rows_host"]
        assert info_without_time(ld) == info
        for a, b in zip(ld.lists(), lists):
            assert np.array_equal(a, b)
        for nq, e in zip((5, 24), expect):
            same(ld.search(q[:nq], K), e, f"host rows nq {nq}")
        assert ld.save() == blob
    finally:
        ld.free()
        seg.free()


def test_part_cache_takes_a_loaded_pair(mq):
    from myscaledb_amd.cache import PartCache
    n, d, nlist = 5000, 64, 8
    rows = O.generate(0x5EED0101, 2, 0, n, d)
    q = O.generate(0x5EED0102, 2, 0, 5, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=1024)
    ref = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    blob = ref.save()
    expect = ref.search(q, K)
    ref.free()
    ld = mq.VectorIndex.load(seg, blob)
    cache = PartCache(1 << 30)
    try:
        cache.put("part_1", seg, ld)
        s2, i2 = cache.acquire("part_1")
        same(i2.search(q, K), expect, "through the cache")
        cache.release("part_1", s2)
    finally:
        cache.free()


def test_np95_survives(mq):
    """n = 2^20 is the smallest part whose build takes the list count (and the
    nprobe reaching recall 0.95, np95) from the data; alpha 3's nprobe derives
    from np95, so the default search probes the same lists after a load."""
    n, d = 1 << 20, 16
    q = O.generate(0x5EED0102, 3, 0, 5, d)
    seg = mq.VectorScanSegment.generate(0x5EED0101, 3, n, d, metric="L2", granule=8192)
    ref = mq.VectorIndex.build(seg, "MSTG")
    ld = None
    try:
        blob = ref.save()
        expect = ref.search(q, K)
        nprobe = mq.vector_index.last_index_stats()["nprobe"]
        ld = mq.VectorIndex.load(seg, blob)
        same(ld.search(q, K), expect, "np95")
        assert mq.vector_index.last_index_stats()["nprobe"] == nprobe
        assert mq.index_blob_info(ld.save())["np95"] == mq.index_blob_info(blob)["np95"]
        assert info_without_time(ld) == info_without_time(ref)
    finally:
        for x in (ld, ref, seg):
            if x is not None:
                x.free()


# ---- the format against the oracle, forged blobs, refusals --------------------

class Saved:
    """One float and one binary part with a saved index each (nlist 8)."""
    n, d, nlist = 5000, 64, 8
    bn, bbits, bnlist = 5000, 136, 7  # (7 x 17 centroid bytes: the assignment starts at an odd offset)

    def __init__(self, mq):
        self.rows = O.generate(0x5EED0101, 2, 0, self.n, self.d)
        self.q = O.generate(0x5EED0102, 2, 0, 24, self.d)
        self.seg = mq.VectorScanSegment.from_rows(self.rows, metric="L2", granule=1024)
        self.idx = mq.VectorIndex.build(self.seg, "MSTG", {"nlist": self.nlist})
        self.blob = self.idx.save()
        self.content = O.decompress_stream(self.blob, len(self.blob), verify=True)
        self.flat = self.seg.search(self.q, K)
        self.codes, self.bq = clustered_codes(11, self.bn, 24, self.bbits // 8)
        self.bseg = mq.BinaryVectorScanSegment.from_codes(self.codes, metric="Hamming", granule=1024)
        self.bidx = mq.BinaryVectorIndex.build(self.bseg, "BINARYMSTG", {"nlist": self.bnlist})
        self.bblob = self.bidx.save()
        self.bcontent = O.decompress_stream(self.bblob, len(self.bblob), verify=True)
        self.bflat = self.bseg.search(self.bq, K)

    def free(self):
        for x in (self.idx, self.seg, self.bidx, self.bseg):
            x.free()


@pytest.fixture(scope="module")
def saved(mq):
    s = Saved(mq)
    yield s
    s.free()


def test_blob_parses_as_documented(mq, saved):
    """decompress_stream(verify=True) checks every block checksum with the
    oracle's CityHash128; then header, centroids and assignment."""
    for blob, content, idx, kind, n, dim, nlist, pad, metric in (
            (saved.blob, saved.content, saved.idx, KIND_FLOAT, saved.n, saved.d, saved.nlist, IVF_PAD, mq._lib.METRIC_L2),
            (saved.bblob, saved.bcontent, saved.bidx, KIND_BINARY, saved.bn, saved.bbits, saved.bnlist, 1,
             mq._lib.METRIC_HAMMING)):
        assert blob[16] == 0x02
        h, cent, assign = split_content(content)
        assert (h["magic"], h["version"], h["kind"], h["metric"], h["dim"], h["n"], h["nlist"], h["alpha"], h["np95"],
                h["reserved"]) == (MAGIC, 1, kind, metric, dim, n, nlist, 3.0, 0, b"\0" * 8)
        assert mq.index_blob_info(blob)["fingerprint"] == h["fingerprint"]
        assert cent == idx.centroids().tobytes()
        assert assign.min() >= 0 and assign.max() < nlist
        off, rows = idx.lists()
        eoff, erows = np_lists(assign, nlist, pad)
        assert np.array_equal(off, eoff) and np.array_equal(rows, erows)


def test_writer_emits_blocks_of_at_most_1mib(mq):
    """A content of more than one block (64 + 4 * 200 * 2048 + 4 * 5000 bytes)."""
    rows = O.generate(0x5EED0101, 2, 0, 5000, 2048)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 200, "kmeans_iters": 1})
    try:
        blob = idx.save()
        content = 64 + 4 * 200 * 2048 + 4 * 5000
        assert content > (1 << 20) and len(blob) == content + 2 * 25
        assert int.from_bytes(blob[21:25], "little") == 1 << 20
        assert len(O.decompress_stream(blob, len(blob), verify=True)) == content
        ld = mq.VectorIndex.load(seg, blob)
        assert ld.save() == blob
        ld.free()
    finally:
        idx.free()
        seg.free()


def forged_assignments(n, nlist, with_none):
    i = np.arange(n)
    edges = (i % nlist).astype(np.int32)  # lists 0, 1, 2 of exactly 15, 16, 17 rows, the rest over the others
    edges[edges < 3] += 3
    pos = np.random.default_rng(5).permutation(n)
    edges[pos[:15]], edges[pos[15:31]], edges[pos[31:48]] = 0, 1, 2
    out = {"one_list": np.full(n, 3, np.int32), "len_15_16_17": edges, "round_robin": (i % nlist).astype(np.int32),
           "descending": (nlist - 1 - i * nlist // n).astype(np.int32)}
    if with_none:
        none = (i % nlist).astype(np.int32)
        none[np.random.default_rng(6).choice(n, 300, replace=False)] = -1
        out["300_in_no_list"] = none
    return out


FORGED_NAMES = ["one_list", "len_15_16_17", "round_robin", "descending"]
FORGED = [("float", name, 0x02) for name in FORGED_NAMES + ["300_in_no_list"]] + \
         [("binary", name, 0x02) for name in FORGED_NAMES] + \
         [("float", "descending", 0x82), ("binary", "one_list", 0x82)]


@pytest.mark.parametrize("kind,name,method", FORGED, ids=[f"{k}_{n}_{'lz4' if m == 0x82 else 'none'}" for k, n, m in FORGED])
def test_forged_assignment_groups_as_a_stable_sort(mq, saved, kind, name, method):
    """Only the assignment section replaced, re-framed by the oracle's writer:
    the lists equal numpy's stable grouping, and a search of every list equals
    FLAT over the rows that are in a list."""
    if kind == "float":
        n, nlist, pad, content, seg, q, cls = saved.n, saved.nlist, IVF_PAD, saved.content, saved.seg, saved.q, mq.VectorIndex
    else:
        n, nlist, pad, content, seg, q, cls = saved.bn, saved.bnlist, 1, saved.bcontent, saved.bseg, saved.bq, mq.BinaryVectorIndex
    assign = forged_assignments(n, nlist, kind == "float")[name]
    if name == "one_list":
        assert n > 4096  # longer than one LDS sort
    if name == "len_15_16_17":
        assert list(np.bincount(assign, minlength=nlist)[:3]) == [15, 16, 17]
    blob = O.compress_stream(with_assignment(content, assign), method=method)
    assert blob[16] == method
    ld = cls.load(seg, blob)
    try:
        off, rows = ld.lists()
        eoff, erows = np_lists(assign, nlist, pad)
        assert np.array_equal(off, eoff)
        assert np.array_equal(rows, erows)
        info = ld.info()
        assert (info["npos"], info["rows_indexed"], info["max_list"]) == \
            (eoff[-1], int((assign >= 0).sum()), int(np.diff(eoff).max()))
        listed = np.packbits((assign >= 0).astype(np.uint8), bitorder="little") if (assign < 0).any() else None
        params = {"nprobe": nlist, "num_reorder": 4096} if kind == "float" else {"nprobe": nlist}
        for nq in (5, 24):
            same(ld.search(q[:nq], K, params, filter_bitmap=listed), seg.search(q[:nq], K, filter_bitmap=listed),
                 f"{kind} {name} nq {nq}")
    finally:
        ld.free()


def refused(mq, cls, seg, blob):
    with pytest.raises(mq._lib.MqvsError) as e:
        cls.load(seg, blob).free()
    return e.value.status


def reframed(content, **kw):
    return O.compress_stream(content, method=0x02, **kw)


def float_refusals(mq, s):
    E = mq._lib
    c, n, d, nlist = s.content, s.n, s.d, s.nlist
    h = parse_header(c)

    def hdr(**kw):
        f = dict(kind=KIND_FLOAT, metric=E.METRIC_L2, dim=d, n=n, nlist=nlist, fingerprint=h["fingerprint"])
        f.update(kw)
        return pack_header(**f) + c[64:]

    def assigned(v):
        a = split_content(c)[2].copy()
        a[n // 2] = v
        return reframed(with_assignment(c, a))

    flipped = bytearray(s.blob)
    flipped[25 + 64 + 1000] ^= 0x10
    bad_method = bytearray(s.blob)
    bad_method[16] = 0x55
    return [
        ("truncated", s.blob[:-10], E.ERR_ILLEGAL_COLUMN),
        ("cut inside the first header", s.blob[:20], E.ERR_ILLEGAL_COLUMN),
        ("unknown method byte", bytes(bad_method), E.ERR_ILLEGAL_COLUMN),
        ("bad magic", reframed(hdr(magic=b"MQVSIDY\0")), E.ERR_ILLEGAL_COLUMN),
        ("4 bytes too many", reframed(c + b"\0" * 4), E.ERR_ILLEGAL_COLUMN),
        ("4 bytes too few", reframed(c[:-4]), E.ERR_ILLEGAL_COLUMN),
        ("assignment = nlist", assigned(nlist), E.ERR_ILLEGAL_COLUMN),
        ("assignment = -2", assigned(-2), E.ERR_ILLEGAL_COLUMN),
        ("assignment = 2^31 - 1", assigned(2 ** 31 - 1), E.ERR_ILLEGAL_COLUMN),
        ("flipped payload bit", bytes(flipped), E.ERR_CHECKSUM),
        ("version 2", reframed(hdr(version=2)), E.ERR_NOT_IMPLEMENTED),
        ("binary blob on a float segment", s.bblob, E.ERR_LOGICAL),
        ("fingerprint", reframed(hdr(fingerprint=h["fingerprint"] ^ 1)), E.ERR_LOGICAL),
    ]


def test_float_refusals_leave_the_segment_usable(mq, saved):
    s = saved
    for what, blob, status in float_refusals(mq, s):
        assert refused(mq, mq.VectorIndex, s.seg, blob) == status, what
        same(s.seg.search(s.q, K), s.flat, f"segment after `{what}`")
        ld = mq.VectorIndex.load(s.seg, s.blob)
        same(ld.search(s.q[:5], K), s.idx.search(s.q[:5], K), f"load after `{what}`")
        ld.free()


def test_binary_refusals_leave_the_segment_usable(mq, saved):
    s, E = saved, mq._lib
    a = split_content(s.bcontent)[2].copy()
    a[7] = -1
    cases = [("binary assignment of -1", reframed(with_assignment(s.bcontent, a)), E.ERR_ILLEGAL_COLUMN),
             ("float blob on a binary segment", s.blob, E.ERR_LOGICAL)]
    a[7] = s.bnlist
    cases.append(("binary assignment = nlist", reframed(with_assignment(s.bcontent, a)), E.ERR_ILLEGAL_COLUMN))
    for what, blob, status in cases:
        assert refused(mq, mq.BinaryVectorIndex, s.bseg, blob) == status, what
        same(s.bseg.search(s.bq, K), s.bflat, f"segment after `{what}`")
        ld = mq.BinaryVectorIndex.load(s.bseg, s.bblob)
        same(ld.search(s.bq[:5], K), s.bidx.search(s.bq[:5], K), f"load after `{what}`")
        ld.free()


def test_blob_of_another_segment_is_refused(mq, saved):
    """n, dimension, cosine / non-cosine family and the rows themselves."""
    s, E = saved, mq._lib
    others = [("other n", s.rows[:4000], "L2"), ("other dimension", np.ascontiguousarray(s.rows[:, :32]), "L2"),
              ("cosine segment", s.rows, "Cosine"), ("other rows", s.rows[::-1].copy(), "L2")]
    for what, rows, metric in others:
        seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=1024)
        try:
            assert refused(mq, mq.VectorIndex, seg, s.blob) == E.ERR_LOGICAL, what
            seg.search(s.q[:5, :rows.shape[1]], K)
        finally:
            seg.free()
    # an IP segment is of the blob's family (not normalised): the same rows load
    seg = mq.VectorScanSegment.from_rows(s.rows, metric="IP", granule=1024)
    ld = mq.VectorIndex.load(seg, s.blob)
    assert ld.info()["metric"] == E.METRIC_L2
    ld.free()
    seg.free()


def test_save_into_a_short_buffer_and_too_wide_a_dimension(mq, saved):
    E = mq._lib
    buf = np.empty(len(saved.blob) - 1, np.uint8)
    written = ctypes.c_size_t(123)
    rc = E.lib.mqvs_index_save(saved.idx._h, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(written))
    assert rc == E.ERR_BAD_ARGUMENTS and written.value == 0
    # wider than the list scan's 16-query tile allows (at most 5056 dimensions): as the build
    n, d = 64, 5120
    rows = O.generate(0x5EED0101, 1, 0, n, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=64)
    try:
        with pytest.raises(E.MqvsError) as e:
            mq.VectorIndex.build(seg, "MSTG", {"nlist": 1})
        assert e.value.status == E.ERR_BAD_ARGUMENTS
        content = pack_header(KIND_FLOAT, E.METRIC_L2, d, n, 1) + b"\0" * (4 * d + 4 * n)
        assert refused(mq, mq.VectorIndex, seg, reframed(content)) == E.ERR_BAD_ARGUMENTS
    finally:
        seg.free()
