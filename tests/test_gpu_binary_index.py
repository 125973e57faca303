"""The binary vector index (BINARYMSTG seam: mqvs_index_build on a binary
segment, mqvs_index_search_binary) on the GPU.

Binary distances are exact integers (Jaccard: one fp32 division of two
integers), so nothing here has a tolerance: an exhaustive index search equals
mqvs_search_binary bit for bit, the build equals a numpy restatement of the
k-majority rule of include/mqvs.h byte for byte, and a partial-nprobe search
equals numpy brute force over exactly the rows of the probed lists.
"""
import ctypes

import numpy as np
import pytest

from kat_harness import check_binary_case, load_binary_cases

pytestmark = pytest.mark.gpu

BCASES = load_binary_cases()
FLT_MAX = np.float32(3.40282347e+38)


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def assert_same(ids_g, dist_g, ids_o, dist_o, ctx):
    ids_g, ids_o = np.asarray(ids_g), np.asarray(ids_o)
    dg, do = np.asarray(dist_g, np.float32).view(np.uint32), np.asarray(dist_o, np.float32).view(np.uint32)
    if not (np.array_equal(ids_g, ids_o) and np.array_equal(dg, do)):
        bad = np.argwhere((ids_g != ids_o) | (dg != do))
        q, j = bad[0]
        raise AssertionError(f"{ctx}: {len(bad)} mismatches; first q{q} slot {j}: index ({ids_g[q, j]}, "
                             f"{dist_g[q, j]!r}) expected ({ids_o[q, j]}, {dist_o[q, j]!r})")


def codes_of(rng, n, nbytes, density=0.5):
    bits = rng.random((n, nbytes * 8)) < density
    return np.packbits(bits, axis=1, bitorder="little")


def clustered(rng, n, nq, nbytes=32, centres=128, density=0.5):
    """centres random codes; rows = a random centre xor Bernoulli(0.10) bit
    noise; queries = rows xor Bernoulli(0.05) noise."""
    cen = codes_of(rng, centres, nbytes, density)
    rows = cen[rng.integers(centres, size=n)] ^ codes_of(rng, n, nbytes, 0.10)
    queries = rows[rng.choice(n, nq, replace=False)] ^ codes_of(rng, nq, nbytes, 0.05)
    return rows, queries


# ---- numpy restatement of the build and the search (include/mqvs.h) ----------

def bits_of(codes):
    return np.unpackbits(np.ascontiguousarray(codes, np.uint8), axis=1, bitorder="little").astype(np.float32)


def hamming(a_bits, b_bits):
    """[len(a), len(b)] Hamming distances (exact in fp32: small integers)."""
    return (a_bits.sum(1)[:, None] + b_bits.sum(1)[None, :] - 2.0 * (a_bits @ b_bits.T)).astype(np.int64)


def np_build(codes, nlist, iters=8):
    """-> (centroid bytes [nlist, N], list of every row, lists left empty in some iteration)."""
    n = len(codes)
    bits = bits_of(codes)
    S = min(n, max(16 * nlist, min(64 * nlist, 1 << 20)))
    samp = bits[(np.arange(S, dtype=np.int64) * n) // S]
    cent = samp[(np.arange(nlist, dtype=np.int64) * S) // nlist].copy()
    empties = 0
    for _ in range(iters):
        a = np.argmin(hamming(samp, cent), axis=1)  # first minimum: the lowest list id
        onehot = np.zeros((nlist, S), np.float32)
        onehot[a, np.arange(S)] = 1.0
        members = onehot.sum(1)
        ones = onehot @ samp
        new = (2.0 * ones > members[:, None]).astype(np.float32)
        empties += int((members == 0).sum())
        cent = np.where(members[:, None] > 0, new, cent)
    assign = np.argmin(hamming(bits, cent), axis=1)
    return np.packbits(cent.astype(np.uint8), axis=1, bitorder="little"), assign, empties


def np_probes(cent_codes, queries, nprobe):
    d = hamming(bits_of(queries), bits_of(cent_codes))
    lists = np.arange(d.shape[1])
    return [set(np.lexsort((lists, d[q]))[:nprobe].tolist()) for q in range(len(queries))]


def np_distances(bits, qbits, metric):
    """float32 [n] of one query, as mqvs_search_binary computes them."""
    inter = bits @ qbits
    if metric == "Hamming":
        return (bits.sum(1) + qbits.sum() - 2.0 * inter).astype(np.float32)
    union = bits.sum(1) + qbits.sum() - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (union - inter).astype(np.float32) / union.astype(np.float32)
    return np.where(inter == 0, np.float32(1.0), v).astype(np.float32)


def np_search(bits, queries, k, metric, rows_ok):
    """Brute force by (distance, row) over the rows rows_ok[q] allows; the
    b < nBit rule and -1 / FLT_MAX padding."""
    nq = len(queries)
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    qb = bits_of(queries)
    nbits = bits.shape[1]
    for q in range(nq):
        d = np_distances(bits, qb[q], metric)
        ok = rows_ok[q].copy()
        if metric == "Hamming":
            ok &= d < nbits
        rows = np.flatnonzero(ok)
        order = rows[np.lexsort((rows, d[rows]))][:k]
        ids[q, :len(order)] = order
        dist[q, :len(order)] = d[order]
    return ids, dist


def bitmap_mask(bm, n):
    return np.ones(n, bool) if bm is None else np.unpackbits(bm, bitorder="little")[:n].astype(bool)


# ---- 1. KAT 00038 through the index -------------------------------------------

@pytest.mark.parametrize("case", BCASES, ids=[c["name"] for c in BCASES])
def test_binary_index_kat(mq, case):
    """A default BINARYMSTG index searched with default params: the 1024-row
    part has 4 lists and nprobe 4, so the golden rows must match exactly."""
    def fn(codes, gran, queries, k, metric, flt, rex):
        seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric, granule=gran)
        idx = mq.BinaryVectorIndex.build(seg)
        try:
            return idx.search(queries, k, None, flt, rex)
        finally:
            idx.free()
            seg.free()
    check_binary_case(case, fn)


# ---- 2. exhaustive == brute force, bitwise --------------------------------------

# (n, bytes per code, nq, k, metric, nlist, filter, deletes, density)
EXHAUSTIVE = [
    (70000, 4, 2, 100, "Hamming", 64, False, False, 0.5),     # heavy ties across lists
    (50000, 136, 9, 20, "Hamming", 64, True, True, 0.5),      # odd width: the row-per-lane form
    (60000, 64, 33, 50, "Jaccard", 128, False, False, 0.3),
    (30000, 128, 5, 30, "Jaccard", 32, True, False, 0.5),
    (3000, 8, 3, 200, "Hamming", 16, True, True, 0.5),        # k > many lists' length
    (40000, 16, 2, 5000, "Hamming", 32, False, False, 0.5),   # k above the LDS sort capacity
]


@pytest.mark.parametrize("n,nb,nq,k,metric,nlist,use_f,use_d,dens", EXHAUSTIVE)
def test_binary_index_exhaustive_equals_brute_force(mq, n, nb, nq, k, metric, nlist, use_f, use_d, dens):
    rng = np.random.default_rng(n + nb + nq + k)
    codes = codes_of(rng, n, nb, dens)
    queries = codes_of(rng, nq, nb, dens)
    queries[0] = codes[n // 3]  # an exact match
    flt = np.packbits(rng.random(n) < 0.4, bitorder="little") if use_f else None
    rex = np.packbits(rng.random(n) > 0.1, bitorder="little") if use_d else None
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
    idx = mq.BinaryVectorIndex.build(seg, params=f"nlist={nlist}")
    try:
        assert idx.info()["rows_indexed"] == n and idx.info()["dim"] == 8 * nb
        ids, dist = idx.search(queries, k, f"nprobe={nlist}", flt, rex)
        ids_b, dist_b = seg.search(queries, k, metric, flt, rex)
    finally:
        idx.free()
        seg.free()
    assert_same(ids, dist, ids_b, dist_b, f"{metric} n={n} N={nb} nq={nq} k={k}")


def test_binary_index_all_ties(mq):
    """Every row at the same distance, more than 4096 of them at the k-th key:
    the smallest rows of the tie group are kept."""
    n = 100000
    seg = mq.BinaryVectorScanSegment.from_codes(np.zeros((n, 32), np.uint8), metric="Hamming")
    idx = mq.BinaryVectorIndex.build(seg, params="nlist=64,kmeans_iters=0")
    q = np.full((1, 32), 0x0F, np.uint8)
    try:
        for k in (10, 600, 4096):
            ids, dist = idx.search(q, k, "nprobe=64")
            assert ids[0].tolist() == list(range(k))
            assert np.all(dist == 128.0)
    finally:
        idx.free()
        seg.free()


# ---- 3 / 4. build and partial-nprobe search pinned -------------------------------

PINNED = [(32768, 32, 128), (32768, 16, 37)]


@pytest.fixture(scope="module", params=PINNED, ids=[f"N{nb}-nlist{L}" for _, nb, L in PINNED])
def pinned(mq, request):
    n, nb, nlist = request.param
    rng = np.random.default_rng(1000 + nb + nlist)
    codes, queries = clustered(rng, n, 16, nb)
    flt = np.packbits(rng.random(n) < 0.4, bitorder="little")
    rex = np.packbits(rng.random(n) > 0.1, bitorder="little")
    cent, assign, empties = np_build(codes, nlist)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    idx = mq.BinaryVectorIndex.build(seg, params=f"nlist={nlist}")
    yield dict(n=n, nlist=nlist, codes=codes, bits=bits_of(codes), queries=queries, flt=flt, rex=rex, cent=cent,
               assign=assign, empties=empties, idx=idx)
    idx.free()
    seg.free()


def test_binary_index_build_pinned(pinned):
    """centroids() equals the numpy restatement byte for byte."""
    # (with as many lists as the data has centres some lists lose every
    # member, so the keep-the-centroid rule is exercised)
    if pinned["nlist"] == 128:
        assert pinned["empties"] > 0
    info = pinned["idx"].info()
    assert info["rows_indexed"] == pinned["n"] and info["nlist"] == pinned["nlist"]
    assert info["npos"] == pinned["n"]
    assert info["max_list"] == np.bincount(pinned["assign"], minlength=pinned["nlist"]).max()
    got = pinned["idx"].centroids()
    assert got.shape == pinned["cent"].shape
    assert np.array_equal(got, pinned["cent"]), f"{(got != pinned['cent']).any(1).sum()} centroids differ"


@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "filter+deletes"])
@pytest.mark.parametrize("nprobe", [1, 3, 16])
def test_binary_index_partial_nprobe_pinned(pinned, nprobe, masked, metric):
    """probes() is the numpy top-nprobe by (Hamming, list id); the result is
    numpy brute force over exactly the rows assigned to a probed list."""
    idx, q, n = pinned["idx"], pinned["queries"], pinned["n"]
    want = np_probes(pinned["cent"], q, nprobe)
    got = idx.probes(q, f"nprobe={nprobe}")
    assert got.shape == (len(q), nprobe)
    assert [set(r.tolist()) for r in got] == want
    flt, rex = (pinned["flt"], pinned["rex"]) if masked else (None, None)
    allowed = bitmap_mask(flt, n) & bitmap_mask(rex, n)
    rows_ok = [allowed & np.isin(pinned["assign"], list(w)) for w in want]
    k = 10
    ids_n, dist_n = np_search(pinned["bits"], q, k, metric, rows_ok)
    ids, dist = idx.search(q, k, f"nprobe={nprobe},metric={metric}", flt, rex)
    assert_same(ids, dist, ids_n, dist_n, f"nprobe={nprobe} {metric} masked={masked}")


def test_binary_index_partial_nprobe_padding(pinned):
    """Fewer than k rows qualify: -1 / FLT_MAX padding after them."""
    idx, q, n = pinned["idx"], pinned["queries"][:4], pinned["n"]
    want = np_probes(pinned["cent"], q, 1)
    keep = np.zeros(n, bool)
    keep[::997] = True
    flt = np.packbits(keep, bitorder="little")
    rows_ok = [keep & np.isin(pinned["assign"], list(w)) for w in want]
    ids_n, dist_n = np_search(pinned["bits"], q, 10, "Hamming", rows_ok)
    assert (ids_n == -1).any()
    ids, dist = idx.search(q, 10, "nprobe=1", flt)
    assert_same(ids, dist, ids_n, dist_n, "padding")


# ---- 5. recall at defaults --------------------------------------------------------

@pytest.mark.parametrize("metric,density", [("Hamming", 0.5), ("Jaccard", 0.3)])
def test_binary_index_recall_defaults(mq, metric, density):
    """recall@10 >= 0.95 (the project's index bar) at the default build and
    search params; a returned row counts when its distance <= the true 10th
    distance (tie-robust)."""
    rng = np.random.default_rng(77)
    codes, queries = clustered(rng, 32768, 64, 32, 128, density)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric)
    idx = mq.BinaryVectorIndex.build(seg)
    try:
        ids, dist = idx.search(queries, 10)
        assert mq.vector_index.last_index_stats()["nprobe"] == 16
        ids_b, dist_b = seg.search(queries, 10)
    finally:
        idx.free()
        seg.free()
    hits = ((ids >= 0) & (dist <= dist_b[:, 9:10])).sum()
    recall = hits / float(ids_b.size)
    print(f"recall@10 {metric}: {recall:.4f}")
    assert recall >= 0.95, recall


# ---- 6. seam behaviour -----------------------------------------------------------

@pytest.fixture(scope="module")
def small(mq):
    rng = np.random.default_rng(5)
    n = 20000
    codes, queries = clustered(rng, n, 8, 32)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    idx = mq.BinaryVectorIndex.build(seg, params="nlist=40")
    yield dict(n=n, codes=codes, queries=queries, seg=seg, idx=idx)
    idx.free()
    seg.free()


def test_binary_index_row_ids_map(small):
    idx, q, n = small["idx"], small["queries"], small["n"]
    ids, dist = idx.search(q, 20, "nprobe=4")
    ids_fs, dist_fs = idx.search(q, 20, "nprobe=4,num_reorder=100", first_stage_only=True)
    assert_same(ids_fs, dist_fs, ids, dist, "first stage == exact result")
    m = (np.arange(n, dtype=np.uint64) * 7 + 3) % np.uint64(n)
    idx.set_row_ids_map(m)
    try:
        ids_m, dist_m = idx.search(q, 20, "nprobe=4")
    finally:
        idx.set_row_ids_map(None)
    assert_same(ids_m, dist_m, np.where(ids >= 0, m[np.maximum(ids, 0)].astype(np.int64), -1), dist, "row_ids_map")


def test_binary_index_device_pointers(small):
    import torch
    idx, q = small["idx"], small["queries"]
    ids, dist = idx.search(q, 20, "nprobe=4")
    ids_d, dist_d = idx.search(torch.from_numpy(q).cuda(), 20, "nprobe=4")
    torch.cuda.synchronize()
    assert_same(ids_d.cpu().numpy(), dist_d.cpu().numpy(), ids, dist, "device pointers")


def test_binary_index_query_sub_batches(small):
    """A batch whose record regions exceed the scratch budget runs in query
    sub-batches: same results and the same probes."""
    from myscaledb_amd._lib import lib
    idx, seg, q = small["idx"], small["seg"], small["queries"]
    ids, dist = idx.search(q, 20, "nprobe=39")
    probes = idx.probes(q, "nprobe=39")
    ids_b, dist_b = seg.search(q, 20)
    prev = lib.mqvs_set_scratch_budget(1 << 20)  # 20000 records of 8 B per query: 6 queries per sub-batch
    try:
        ids_s, dist_s = idx.search(q, 20, "nprobe=39")
        probes_s = idx.probes(q, "nprobe=39")
        ids_e, dist_e = idx.search(q, 20, "nprobe=40")
    finally:
        lib.mqvs_set_scratch_budget(prev)
    assert_same(ids_s, dist_s, ids, dist, "sub-batched search")
    assert [set(r) for r in probes_s.tolist()] == [set(r) for r in probes.tolist()]
    assert_same(ids_e, dist_e, ids_b, dist_b, "sub-batched exhaustive search")


def test_binary_index_async(mq, small):
    """An ASYNC device-pointer search into preallocated outputs: nothing is
    flagged, and the ids and distance bits are the synchronous host-pointer
    search's, with and without a row-ids map."""
    import torch
    idx, q, n = small["idx"], small["queries"], small["n"]
    ids, dist = idx.search(q, 20, "nprobe=4")
    dq = torch.from_numpy(q).cuda()
    out = (torch.empty((len(q), 20), dtype=torch.int64, device="cuda"),
           torch.empty((len(q), 20), dtype=torch.float32, device="cuda"))

    def run_async(ctx, want_ids):
        out[0].fill_(-7)
        out[1].fill_(-7.0)
        torch.cuda.synchronize()  # (the search runs on the library's stream)
        got = idx.search(dq, 20, "nprobe=4", out=out, async_=True)
        torch.cuda.synchronize()
        mq.vector_scan.async_check()
        assert got[0] is out[0] and got[1] is out[1]
        assert_same(out[0].cpu().numpy(), out[1].cpu().numpy(), want_ids, dist, ctx)

    run_async("async", ids)
    m = (np.arange(n, dtype=np.uint64) * 7 + 3) % np.uint64(n)
    idx.set_row_ids_map(m)
    try:
        run_async("async, row_ids_map", np.where(ids >= 0, m[np.maximum(ids, 0)].astype(np.int64), -1))
    finally:
        idx.set_row_ids_map(None)


def test_binary_index_sub_batch_stats(mq, small):
    """The stats of a sub-batched search are the sums over its sub-batches:
    k_bivf_stats adds values, items, plane_bytes and pairs per (query, probe)
    pair, so they equal the unbatched search's."""
    from myscaledb_amd._lib import lib
    idx, q = small["idx"], small["queries"]
    idx.search(q, 20, "nprobe=39")
    whole = mq.vector_index.last_index_stats()
    prev = lib.mqvs_set_scratch_budget(1 << 20)  # 6 queries per sub-batch, as test_binary_index_query_sub_batches
    try:
        idx.search(q, 20, "nprobe=39")
        st = mq.vector_index.last_index_stats()
    finally:
        lib.mqvs_set_scratch_budget(prev)
    assert st["nq"] == len(q) and st["k"] == 20 and st["nprobe"] == 39
    assert st["pairs"] == 39 * len(q)
    for f in ("values", "items", "plane_bytes", "pairs"):
        assert st[f] == whole[f], (f, st[f], whole[f])
    assert st["values"] > 0 and st["plane_bytes"] > 0
    assert st["rerank_ms"] == 0 and st["reranked"] == 0


def test_binary_index_stats(mq, small):
    idx, q = small["idx"], small["queries"]
    idx.search(q, 20, "nprobe=4")
    st = mq.vector_index.last_index_stats()
    assert st["nprobe"] == 4 and st["nq"] == len(q) and st["k"] == 20
    assert st["pairs"] == 4 * len(q) and st["values"] > 0 and st["plane_bytes"] > 0
    assert st["rerank_ms"] == 0 and st["reranked"] == 0


def test_binary_index_through_cache(mq):
    from myscaledb_amd._lib import check, lib
    from myscaledb_amd.vector_scan import _ptr
    rng = np.random.default_rng(6)
    codes, q = clustered(rng, 5000, 4, 16)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Jaccard")
    idx = mq.BinaryVectorIndex.build(seg, params="nlist=8")
    want_ids, want_dist = seg.search(q, 15)
    cache = ctypes.c_void_p()
    check(lib.mqvs_cache_create(1 << 30, ctypes.byref(cache)))
    try:
        check(lib.mqvs_cache_put(cache, b"part", seg._h, idx._h))
        seg._h = idx._h = None  # the cache owns both now
        s, i = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.mqvs_cache_acquire(cache, b"part", ctypes.byref(s), ctypes.byref(i)))
        assert s.value and i.value
        ids = np.empty((4, 15), np.int64)
        dist = np.empty((4, 15), np.float32)
        check(lib.mqvs_index_search_binary(i, _ptr(q), 4, 15, b"nprobe=8", None, None, _ptr(ids), _ptr(dist), 0, None))
        check(lib.mqvs_cache_release(cache, b"part", s))
    finally:
        check(lib.mqvs_cache_free(cache))
    assert_same(ids, dist, want_ids, want_dist, "acquired handles")


# ---- 7. errors ---------------------------------------------------------------------

def test_binary_index_errors(mq, small):
    from myscaledb_amd import _lib
    from myscaledb_amd._lib import lib
    from myscaledb_amd.vector_scan import _ptr
    seg, idx, q = small["seg"], small["idx"], small["queries"]

    def status_of(fn):
        with pytest.raises(_lib.MqvsError) as e:
            fn()
        return e.value.status

    fseg = mq.VectorScanSegment.from_rows(np.random.default_rng(1).random((512, 16), np.float32), metric="L2")
    fidx = mq.VectorIndex.build(fseg, params="nlist=4")
    try:
        # index type vs segment kind
        assert status_of(lambda: mq.BinaryVectorIndex.build(seg, "MSTG")) == _lib.ERR_LOGICAL
        assert status_of(lambda: mq.VectorIndex.build(fseg, "BINARYMSTG")) == _lib.ERR_LOGICAL
        assert status_of(lambda: mq.VectorIndex.build(fseg, "binaryivf")) == _lib.ERR_LOGICAL
        # query kind vs index kind
        ids = np.empty((1, 5), np.int64)
        dist = np.empty((1, 5), np.float32)
        fq = np.zeros((1, 256), np.float32)
        assert lib.mqvs_index_search(idx._h, _ptr(fq), 1, 5, b"", None, None, _ptr(ids), _ptr(dist), 0,
                                     None) == _lib.ERR_LOGICAL
        assert lib.mqvs_index_search_binary(fidx._h, _ptr(q), 1, 5, b"", None, None, _ptr(ids), _ptr(dist), 0,
                                            None) == _lib.ERR_LOGICAL
        # parameters
        assert status_of(lambda: mq.BinaryVectorIndex.build(seg, params="nlist=8,foo=1")) == _lib.ERR_BAD_ARGUMENTS
        assert status_of(lambda: idx.search(q, 5, "foo=1")) == _lib.ERR_BAD_ARGUMENTS
        assert status_of(lambda: mq.BinaryVectorIndex.build(seg, params=f"nlist={small['n'] + 1}")) == \
            _lib.ERR_BAD_ARGUMENTS
        assert status_of(lambda: idx.search(q, 5, "nprobe=41")) == _lib.ERR_BAD_ARGUMENTS
        assert status_of(lambda: idx.search(q[:, :16], 5)) == _lib.ERR_LOGICAL
        assert status_of(lambda: idx.probes(q[:, :16])) == _lib.ERR_LOGICAL
        assert status_of(lambda: idx.search(q, 5, "metric=L2")) == _lib.ERR_NOT_IMPLEMENTED
        assert status_of(lambda: mq.BinaryVectorIndex.build(seg, params="metric_type=L2")) == \
            _lib.ERR_NOT_IMPLEMENTED
    finally:
        fidx.free()
        fseg.free()
    # a BINARYIVF index of the other metric on the same segment
    jidx = mq.BinaryVectorIndex.build(seg, "binaryivf", "nlist=40,metric_type=Jaccard")
    try:
        assert jidx.info()["metric"] == _lib.METRIC_JACCARD
        ids_j, dist_j = jidx.search(q, 5, "nprobe=40")
        ids_b, dist_b = seg.search(q, 5, "Jaccard")
    finally:
        jidx.free()
    assert_same(ids_j, dist_j, ids_b, dist_b, "Jaccard index on a Hamming segment")
