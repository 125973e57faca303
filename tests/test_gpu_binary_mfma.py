"""The i8 MFMA route of binary vectors (kernels_binary_mfma.hip): the opt-in
batch scan of mqvs_search_binary (mqvs_set_binary_batch) and the opt-in
assignment kernel of the binary index build (assign=mfma).

With the code bits as 0/1 bytes the i32 accumulator holds popcount(x & q)
exactly and both distances are integer expressions of it, so nothing here has
a tolerance: ids and distance bits equal the CPU oracle's and the popcount
route's on the same segment, and the built index equals the assign=valu one.
"""
import contextlib

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_binary_index import bits_of, clustered, hamming, np_build

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.40282347e+38)
METRICS = ["Hamming", "Jaccard"]


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


@contextlib.contextmanager
def batch_route(mq, min_nq):
    prev = mq.set_binary_batch(min_nq)
    try:
        yield
    finally:
        mq.set_binary_batch(prev)


def assert_same(ids_g, dist_g, ids_o, dist_o, ctx):
    ids_g, ids_o = np.asarray(ids_g), np.asarray(ids_o)
    dg, do = np.asarray(dist_g, np.float32).view(np.uint32), np.asarray(dist_o, np.float32).view(np.uint32)
    if not (np.array_equal(ids_g, ids_o) and np.array_equal(dg, do)):
        bad = np.argwhere((ids_g != ids_o) | (dg != do))
        q, j = bad[0]
        raise AssertionError(f"{ctx}: {len(bad)} mismatches; first q{q} slot {j}: got ({ids_g[q, j]}, "
                             f"{dist_g[q, j]!r}) expected ({ids_o[q, j]}, {dist_o[q, j]!r})")


def codes_of(rng, n, nbytes, density=0.5):
    bits = rng.random((n, nbytes * 8)) < density
    return np.packbits(bits, axis=1, bitorder="little")


def stats():
    from myscaledb_amd import _lib
    return _lib.last_search_stats()


def check_routes(mq, seg, codes, queries, k, metric, ctx, flt=None, rex=None, gran=8192, min_nq=1):
    """The MFMA route == the oracle == the popcount route on the same segment.
    Returns the MFMA route's stats."""
    ids_p, dist_p = seg.search(queries, k, metric, flt, rex)
    assert stats()["path"] == 3
    with batch_route(mq, min_nq):
        ids, dist = seg.search(queries, k, metric, flt, rex)
        st = stats()
    ids_o, dist_o = O.vector_scan_binary(codes, queries, k, O.METRICS[metric], gran, filter_bits=flt,
                                         row_exists_bits=rex)
    assert_same(ids, dist, ids_o, dist_o, f"mfma vs oracle: {ctx}")
    assert_same(ids, dist, ids_p, dist_p, f"mfma vs popcount: {ctx}")
    return st


# ---- 1. settings ---------------------------------------------------------------

def test_setting_round_trip_and_path(mq):
    from myscaledb_amd import _lib
    assert mq.binary_batch() == 0
    rng = np.random.default_rng(1)
    codes, q = codes_of(rng, 500, 32), codes_of(rng, 20, 32)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    try:
        seg.search(q, 5)
        assert stats()["path"] == 3
        with batch_route(mq, 20):
            assert mq.binary_batch() == 20
            assert _lib.lib.mqvs_set_binary_batch(-1) == _lib.ERR_BAD_ARGUMENTS
            assert mq.binary_batch() == 20
            _lib.check(_lib.lib.mqvs_binary_batch(None))
            seg.search(q, 5)
            assert stats()["path"] == 4
            seg.search(q[:19], 5)
            assert stats()["path"] == 3
            assert mq.set_binary_batch(7) == 20
            assert mq.binary_batch() == 7
            seg.search(q[:7], 5)
            assert stats()["path"] == 4
        assert mq.binary_batch() == 0
        seg.search(q, 5)
        assert stats()["path"] == 3
    finally:
        seg.free()
        mq.set_binary_batch(0)


# ---- 2. results == oracle == popcount route --------------------------------------

ROWS = [1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 3000]   # the 16-row block, the 64 / 256-row tiles +- 1
BATCHES = [1, 15, 16, 17, 20, 33, 129, 257]                  # the column block, the 32 / 64 / 128 tiles +- 1


@pytest.mark.parametrize("metric", METRICS)
def test_row_and_batch_edges(mq, metric):
    rng = np.random.default_rng(11)
    allq = codes_of(rng, max(BATCHES), 32, 0.4)
    for n in ROWS:
        codes = codes_of(rng, n, 32, 0.4)
        if n > 2:
            allq[0] = codes[n // 3]   # an exact match
            codes[n - 1] = ~allq[min(BATCHES) - 1]  # a complement
        seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
        try:
            for nq in BATCHES:
                st = check_routes(mq, seg, codes, allq[:nq], 10, metric, f"{metric} n={n} nq={nq}")
                assert st["path"] == 4 and st["nq"] == nq
        finally:
            seg.free()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nb", [4, 8, 16, 17, 32, 64, 128, 136])
def test_code_widths(mq, nb, metric):
    """sub-16-byte, odd and > 1024-bit codes (the plane streamed in K chunks)."""
    rng = np.random.default_rng(100 + nb)
    n = 3000
    codes = codes_of(rng, n, nb, 0.35)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
    try:
        for nq in (33, 129):
            q = codes_of(rng, nq, nb, 0.35)
            q[1] = codes[7]
            check_routes(mq, seg, codes, q, 25, metric, f"{metric} N={nb} nq={nq}")
    finally:
        seg.free()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [20, 64, 200])
def test_probe_segments_and_refines(mq, nq, metric):
    """A part past the dense limit: the APPEND epilogue and the refines run."""
    rng = np.random.default_rng(70000 + nq)
    n = 70000
    codes, q = codes_of(rng, n, 32), codes_of(rng, nq, 32)
    q[0] = codes[n - 5]
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
    try:
        st = check_routes(mq, seg, codes, q, 100, metric, f"{metric} 70000 x 32 B nq={nq}")
        assert st["path"] == 4
        assert st["probe_rows"] < n and st["segments"] >= 1
    finally:
        seg.free()


@pytest.mark.parametrize("metric", METRICS)
def test_heavy_ties_4_byte_codes(mq, metric):
    rng = np.random.default_rng(4)
    n = 70000
    codes, q = codes_of(rng, n, 4), codes_of(rng, 24, 4)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
    try:
        st = check_routes(mq, seg, codes, q, 100, metric, f"{metric} 32-bit codes")
        assert st["probe_rows"] < n and st["segments"] >= 1
    finally:
        seg.free()


@pytest.mark.parametrize("metric", METRICS)
def test_filter_and_deletes(mq, metric):
    rng = np.random.default_rng(40)
    n, gran = 50000, 1000
    codes, q = codes_of(rng, n, 16, 0.3), codes_of(rng, 33, 16, 0.3)
    flt = np.packbits(rng.random(n) < 0.4, bitorder="little")
    rex = np.packbits(rng.random(n) > 0.1, bitorder="little")
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric, granule=gran)
    try:
        check_routes(mq, seg, codes, q, 64, metric, f"{metric} filter+deletes", flt, rex, gran)
        check_routes(mq, seg, codes, q, 64, metric, f"{metric} filter", flt, None, gran)
    finally:
        seg.free()


def test_large_k_sub_batches(mq):
    """k > 4096: search_binary's query sub-batches each take the route."""
    rng = np.random.default_rng(5000)
    n = 40000
    codes, q = codes_of(rng, n, 16), codes_of(rng, 40, 16)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    try:
        check_routes(mq, seg, codes, q, 5000, "Hamming", "k=5000")
    finally:
        seg.free()


@pytest.mark.parametrize("metric", METRICS)
def test_asymmetric_rows_and_queries(mq, metric):
    """Row r is a prefix of r 7 mod 257 ones, query j the bits b with
    b (j + 2) mod 5 == 0 shifted by j: the value of (r, j) is not the value of
    any (j', r') a row <-> column swap inside a tile could write."""
    nbits, n, nq = 256, 300, 40
    pos = np.arange(nbits)
    rows = (pos[None, :] < ((np.arange(n) * 7) % 257)[:, None])
    qs = ((pos[None, :] * (np.arange(nq)[:, None] + 2)) % 5 == 0) & (pos[None, :] >= np.arange(nq)[:, None])
    a, b = rows.astype(np.int64), qs.astype(np.int64)
    d = a.sum(1)[:, None] + b.sum(1)[None, :] - 2 * (a @ b.T)
    assert not np.array_equal(d[:nq, :nq], d[:nq, :nq].T)
    codes = np.packbits(rows, axis=1, bitorder="little")
    q = np.packbits(qs, axis=1, bitorder="little")
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
    try:
        check_routes(mq, seg, codes, q, 300, metric, f"{metric} asymmetric")
    finally:
        seg.free()


# ---- 3. value rules ----------------------------------------------------------------

def test_complement_rows(mq):
    rng = np.random.default_rng(9)
    n, nq = 400, 24
    codes, q = codes_of(rng, n, 16), codes_of(rng, nq, 16)
    for j in range(nq):
        codes[17 * j + 3] = ~q[j]
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    try:
        with batch_route(mq, 1):
            ids, dist = seg.search(q, n, "Hamming")
            assert stats()["path"] == 4
            idj, distj = seg.search(q, n, "Jaccard")
        for j in range(nq):
            r = 17 * j + 3
            assert r not in ids[j].tolist(), f"query {j}: the complement row is at distance nbits"
            assert (ids[j] >= 0).sum() == n - 1 and ids[j, -1] == -1 and dist[j, -1] == FLT_MAX
            at = idj[j].tolist().index(r)
            assert distj[j, at] == np.float32(1.0)
        check_routes(mq, seg, codes, q, n, "Hamming", "complements")
        check_routes(mq, seg, codes, q, n, "Jaccard", "complements")
    finally:
        seg.free()


def test_jaccard_zero_numerator(mq):
    """num == 0 both ways: an all-zero row against any query, any row against an
    all-zero query (den 0 included) -> 1.0."""
    rng = np.random.default_rng(10)
    n, nq = 300, 20
    codes, q = codes_of(rng, n, 8, 0.5), codes_of(rng, nq, 8, 0.5)
    codes[::7] = 0
    q[5] = 0
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Jaccard")
    try:
        with batch_route(mq, 1):
            ids, dist = seg.search(q, n, "Jaccard")
        assert np.all(dist[5] == np.float32(1.0)) and ids[5].tolist() == list(range(n))
        for j in (0, 19):
            zero_rows = np.isin(ids[j], np.arange(0, n, 7))
            assert np.all(dist[j][zero_rows] == np.float32(1.0))
        check_routes(mq, seg, codes, q, n, "Jaccard", "zero numerators")
    finally:
        seg.free()


def test_all_ties(mq):
    """100 000 identical rows: rows 0 .. k-1, also when more than 4096 rows
    reach the k-th distance."""
    n, nq = 100000, 32
    codes = np.zeros((n, 32), np.uint8)
    q = np.full((nq, 32), 0x0F, np.uint8)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    try:
        with batch_route(mq, 20):
            for k in (10, 600, 4096):
                ids, dist = seg.search(q, k)
                assert stats()["path"] == 4
                assert np.array_equal(ids, np.tile(np.arange(k), (nq, 1)))
                assert np.all(dist == 128.0)
    finally:
        seg.free()


# ---- 4. device pointers, ASYNC -------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_device_pointers_and_async(mq, metric):
    import torch
    rng = np.random.default_rng(3)
    n, nb, nq, k = 40960, 32, 48, 50
    codes, q = codes_of(rng, n, nb), codes_of(rng, nq, nb)
    ids_o, dist_o = O.vector_scan_binary(codes, q, k, O.METRICS[metric], 8192)
    tc, tq = torch.from_numpy(codes).cuda(), torch.from_numpy(q).cuda()
    seg = mq.BinaryVectorScanSegment.from_codes(tc, metric=metric)
    try:
        with batch_route(mq, 20):
            ids, dist = seg.search(tq, k)
            assert stats()["path"] == 4
            assert_same(ids.cpu().numpy(), dist.cpu().numpy(), ids_o, dist_o, "device pointers")
            out = (torch.full((nq, k), -7, dtype=torch.int64, device="cuda"),
                   torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda"))
            torch.cuda.synchronize()  # (the search runs on the library's stream)
            got = seg.search(tq, k, out=out, async_=True)
            torch.cuda.synchronize()
            mq.vector_scan.async_check()
            assert got[0] is out[0] and got[1] is out[1]
            assert_same(out[0].cpu().numpy(), out[1].cpu().numpy(), ids_o, dist_o, "async")
    finally:
        seg.free()


# ---- 5. index build: assign=mfma ------------------------------------------------------

def index_pair(mq, codes, params):
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    valu = mq.BinaryVectorIndex.build(seg, params=dict(params, assign="valu"))
    mfma = mq.BinaryVectorIndex.build(seg, params=dict(params, assign="mfma"))
    return seg, valu, mfma


def assert_same_index(valu, mfma, ctx):
    assert np.array_equal(mfma.centroids(), valu.centroids()), f"{ctx}: centroids differ"
    off_v, rows_v = valu.lists()
    off_m, rows_m = mfma.lists()
    assert np.array_equal(off_m, off_v), f"{ctx}: list offsets differ"
    assert np.array_equal(rows_m, rows_v), f"{ctx}: list rows differ"


@pytest.mark.parametrize("n,nb,nlist", [(32768, 32, 128), (32768, 16, 37), (5000, 136, 16)])
def test_build_assign_mfma_equals_valu(mq, n, nb, nlist):
    rng = np.random.default_rng(1000 + nb + nlist)
    codes, queries = clustered(rng, n, 16, nb)
    cent, assign, _ = np_build(codes, nlist)
    seg, valu, mfma = index_pair(mq, codes, {"nlist": nlist})
    try:
        assert_same_index(valu, mfma, f"n={n} N={nb} nlist={nlist}")
        assert np.array_equal(mfma.centroids(), cent), "centroids differ from the numpy restatement"
        off, rows = mfma.lists()
        got = np.empty(n, np.int64)
        got[rows] = np.repeat(np.arange(nlist), np.diff(off))
        assert np.array_equal(got, assign), "assignment differs from the numpy restatement"
        flt = np.packbits(rng.random(n) < 0.4, bitorder="little")
        rex = np.packbits(rng.random(n) > 0.1, bitorder="little")
        for nprobe in (1, 3, nlist):
            for metric in METRICS:
                p = f"nprobe={nprobe},metric={metric}"
                a, b = valu.search(queries, 10, p), mfma.search(queries, 10, p)
                assert_same(b[0], b[1], a[0], a[1], f"search {p}")
                a, b = valu.search(queries, 10, p, flt, rex), mfma.search(queries, 10, p, flt, rex)
                assert_same(b[0], b[1], a[0], a[1], f"masked search {p}")
    finally:
        for x in (valu, mfma, seg):
            x.free()


def test_build_with_empty_lists(mq):
    """Three distinct codes, 16 lists: the duplicates of a centroid lose every
    member to the lowest list and keep their centroid."""
    rng = np.random.default_rng(77)
    three = codes_of(rng, 3, 32)
    codes = three[np.arange(60) % 3]
    seg, valu, mfma = index_pair(mq, codes, {"nlist": 16})
    try:
        assert_same_index(valu, mfma, "empty lists")
        off, _ = mfma.lists()
        assert (np.diff(off) == 0).sum() >= 13
        cent, assign, empties = np_build(codes, 16)
        assert empties > 0 and np.array_equal(mfma.centroids(), cent)
    finally:
        for x in (valu, mfma, seg):
            x.free()


def test_build_tie_goes_to_the_lower_list(mq):
    """130 lists of 3 identical rows each (the initial centroids are those
    codes, and stay), plus one row equidistant from the codes of lists 3 and
    129 -- two column tiles apart -- and of lists 40 and 41, inside one
    16-column block: each lands in the lower list."""
    rng = np.random.default_rng(130)
    L, m, nb = 130, 3, 32
    cen = codes_of(rng, L, nb)

    def between(i, j):
        diff = np.flatnonzero(np.unpackbits(cen[i] ^ cen[j], bitorder="little"))
        if len(diff) % 2:  # make the distance even
            cen[j, diff[-1] // 8] ^= np.uint8(1 << (diff[-1] % 8))
            diff = diff[:-1]
        x = np.unpackbits(cen[i], bitorder="little")
        x[diff[: len(diff) // 2]] ^= 1
        return np.packbits(x, bitorder="little")

    x0, x1 = between(3, 129), between(40, 41)
    codes = np.concatenate([np.repeat(cen, m, axis=0), x0[None], x1[None]])
    n = len(codes)
    d = hamming(bits_of(codes[-2:]), bits_of(cen))
    assert d[0, 3] == d[0, 129] == d[0].min() and (d[0] == d[0].min()).sum() == 2
    assert d[1, 40] == d[1, 41] == d[1].min() and (d[1] == d[1].min()).sum() == 2
    seg, valu, mfma = index_pair(mq, codes, {"nlist": L, "sample": n})
    try:
        assert_same_index(valu, mfma, "ties")
        assert np.array_equal(mfma.centroids(), cen)
        off, rows = mfma.lists()
        assert rows[off[3]:off[4]].tolist() == [9, 10, 11, n - 2]
        assert rows[off[40]:off[41]].tolist() == [120, 121, 122, n - 1]
        assert rows[off[129]:off[130]].tolist() == [387, 388, 389]
    finally:
        for x in (valu, mfma, seg):
            x.free()


def test_build_assign_errors(mq):
    from myscaledb_amd import _lib
    codes = codes_of(np.random.default_rng(0), 200, 16)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    fseg = mq.VectorScanSegment.from_rows(np.ones((200, 16), np.float32), metric="L2")
    try:
        with pytest.raises(_lib.MqvsError) as e:
            mq.BinaryVectorIndex.build(seg, params={"nlist": 4, "assign": "bogus"})
        assert e.value.status == _lib.ERR_BAD_ARGUMENTS
        with pytest.raises(_lib.MqvsError) as e:
            mq.VectorIndex.build(fseg, params={"nlist": 4, "assign": "mfma"})
        assert e.value.status == _lib.ERR_BAD_ARGUMENTS
    finally:
        seg.free()
        fseg.free()
