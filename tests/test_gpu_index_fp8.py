"""The fp8 list plane of the float index (mqvs_index_build, plane=fp8) on the GPU.

The plane stores OCP e4m3fn codes with one power-of-two scale per list
position; the list scan sums the code products in fp32.  Only the candidate set and the
size of the pruning bound may differ from a bf16 index: every returned
distance is the exact fp32 one.  So the tests pin

* the format (mqvs_index_plane, hbm_bytes, parameter errors),
* the first stage's arithmetic against a numpy restatement of the quantiser
  of include/mqvs.h (numpy only: frexp exponent, rint for round-to-nearest-even,
  4 significant bits for normals, step 2^-9 below 2^-6),
* exhaustive search == FLAT bit for bit with the pruning on, in grouped mode
  with 16-, 32- and 64-query tiles, in pair mode, over ragged lists and over
  the value classes of value_cases.py,
* recall at the default parameters, save / load, and rows in host memory.

Every test builds with plane=fp8.
"""
import numpy as np
import pytest

import value_cases as V
from index_blob_format import parse_header
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FP8 = {"plane": "fp8"}
U = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def same_bits(a, b, ctx):
    (ia, da), (ib, db) = a, b
    assert np.array_equal(ia, ib), ctx
    assert np.array_equal(np.asarray(da, np.float32).view(np.uint32), np.asarray(db, np.float32).view(np.uint32)), ctx


# ---- the quantiser of include/mqvs.h, restated ------------------------------

def e4m3_round(v):
    """The e4m3fn value nearest to each finite |v| <= 448 (float64), ties to even."""
    a = np.abs(v)
    _, ex = np.frexp(a)                                  # a = m 2^ex, m in [0.5, 1)
    step = np.ldexp(1.0, np.maximum(ex - 4, -9))         # 4 significant bits; 2^-9 below 2^-6
    return np.sign(v) * np.rint(a / step) * step


def quantise(x):
    """(the de-scaled code vectors as float64, the scale exponents) of fp32 rows."""
    x = np.asarray(x, np.float32)
    amax = np.abs(x).max(axis=1)
    _, E = np.frexp(amax)
    e = np.where(np.isfinite(amax) & (amax > 0), 8 - E, 0).astype(np.int64)
    scaled = np.ldexp(x.astype(np.float64), e[:, None])
    assert np.all(np.abs(scaled) < 256)
    return np.ldexp(e4m3_round(scaled), -e[:, None]), e


def check_restatement():
    """The restatement itself: the 127 non-negative e4m3fn values are fixed
    points, midpoints go to the even neighbour, and a row's scaled maximum
    lands in [128, 256)."""
    vals = np.array([m * 2.0 ** -9 for m in range(8)] +
                    [(8 + m) * 2.0 ** (e - 10) for e in range(1, 16) for m in range(8)][:-1])
    assert vals.size == 127 and vals.max() == 448 and np.all(np.diff(vals) > 0)
    assert np.array_equal(e4m3_round(vals), vals) and np.array_equal(e4m3_round(-vals), -vals)
    mid = (vals[:-1] + vals[1:]) / 2
    even = np.where(np.arange(126) % 2 == 0, vals[:-1], vals[1:])  # codes with an even mantissa
    assert np.array_equal(e4m3_round(mid), even)
    y8, e = quantise(np.array([[0.3, -1.7, 0.01], [0, 0, 0], [1e-20, 3e-21, 0]], np.float32))
    assert list(e) == [7, 0, 74]
    assert np.abs(np.ldexp(y8, e[:, None])).max(axis=1).tolist() == [224.0, 0.0, 192.0]


def bf16_round(x):
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def approx_reference(rows, q, metric):
    """What the fp8 first stage computes, in float64: (value[nq, n] in the
    metric's first-stage form, sum |x8_i y8_i| [nq, n], qn + pn [nq, n] (L2))."""
    if metric == "Cosine":
        rows, q = O.normalize(rows), O.normalize(q)
    y8, _ = quantise(rows)
    x8, _ = quantise(q)
    ip = x8 @ y8.T
    mag = np.abs(x8) @ np.abs(y8).T
    npn = None
    if metric == "L2":
        # (the fp32 norms the search keeps: the reference's fvec_norm_L2sqr)
        qn = np.array([O.norm_l2sqr(v) for v in q], np.float64)
        pn = np.array([O.norm_l2sqr(v) for v in rows], np.float64)
        npn = qn[:, None] + pn[None, :]
        return npn - 2 * ip, mag, npn
    return (1 - ip if metric == "Cosine" else ip), mag, npn


def tolerance(metric, d, value, mag, npn):
    """The MFMA accumulation bound of kernels_bf16.hip (2.04 d u sum |p|) on the
    fp8 products, plus the roundings of the metric's final form."""
    t = 2.04 * d * U * mag
    if metric == "L2":
        return 2 * t + 2.4e-7 * npn
    if metric == "Cosine":
        return t + 2.4e-7
    return t + np.abs(value) * 2.0 ** -23


# ---- 1. the format is real ---------------------------------------------------

def test_format_and_bytes(mq):
    n, d, nlist = 3000, 100, 8
    rows = O.generate(0x5EED0001, 2, 0, n, d)
    q = O.generate(0x5EED0002, 2, 0, 24, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=1024)
    built = []
    try:
        f8 = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
        built.append(f8)
        up = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "FP8"})
        built.append(up)
        b16 = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "bf16"})
        built.append(b16)
        dflt = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
        built.append(dflt)
        info8, info16 = f8.info(), b16.info()
        npos, dpad = info8["npos"], 128
        assert info16["npos"] == npos and npos % 16 == 0 and npos >= n
        scale_bytes = 2 * npos  # int16 per position
        assert f8.plane() == {"format": 1, "plane_bytes": npos * dpad + scale_bytes}
        assert up.plane() == f8.plane()
        assert b16.plane() == {"format": 0, "plane_bytes": 2 * npos * dpad}
        assert dflt.plane() == b16.plane()
        assert info16["hbm_bytes"] - info8["hbm_bytes"] == npos * dpad - scale_bytes
        assert dflt.info()["hbm_bytes"] == info16["hbm_bytes"]
        for a, b in zip(f8.lists(), b16.lists()):
            assert np.array_equal(a, b)
        # the coarse quantizer is not fp8: the same probes
        assert np.array_equal(np.sort(f8.probes(q, {"nprobe": 3}), axis=1), np.sort(b16.probes(q, {"nprobe": 3}), axis=1))
        for kw in ({}, {"first_stage_only": True}):
            same_bits(b16.search(q, 20, {"nprobe": 3}, **kw), dflt.search(q, 20, {"nprobe": 3}, **kw), f"bf16 {kw}")
        # the scan reports the bytes it streams: half the bf16 scan's at equal probes
        f8.search(q, 20, {"nprobe": 3})
        st8 = mq.vector_index.last_index_stats()
        b16.search(q, 20, {"nprobe": 3})
        st16 = mq.vector_index.last_index_stats()
        assert st8["values"] == st16["values"] and st8["plane_bytes"] > 0
        assert 2 * st8["plane_bytes"] == st16["plane_bytes"]
        with pytest.raises(mq._lib.MqvsError, match="BAD_ARGUMENTS"):
            mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "int4"})
    finally:
        for ix in built:
            ix.free()
        seg.free()


def test_binary_index_rejects_the_key(mq):
    codes = np.random.default_rng(3).integers(0, 256, (500, 16), dtype=np.uint8)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    try:
        with pytest.raises(mq._lib.MqvsError, match="BAD_ARGUMENTS.*`plane`"):
            mq.BinaryVectorIndex.build(seg, "BINARYMSTG", {"nlist": 4, "plane": "fp8"})
        idx = mq.BinaryVectorIndex.build(seg, "BINARYMSTG", {"nlist": 4})
        try:
            import ctypes
            fmt, nb = ctypes.c_int32(), ctypes.c_size_t()
            assert mq._lib.lib.mqvs_index_plane(idx._h, ctypes.byref(fmt), ctypes.byref(nb)) == mq._lib.ERR_LOGICAL
        finally:
            idx.free()
    finally:
        seg.free()


# ---- 2. the first stage pins the arithmetic ----------------------------------

FIRST_STAGE = [(d, m) for d in (64, 100, 768) for m in ("L2", "IP", "Cosine")]


@pytest.mark.parametrize("d,metric", FIRST_STAGE, ids=[f"d{d}-{m}" for d, m in FIRST_STAGE])
def test_first_stage_values(mq, d, metric):
    """Every value the first stage returns is the numpy reference's (float64
    dot of the de-scaled fp8 row and query) within the MFMA accumulation
    bound, the k-th returned value is the reference's k-th best, and some
    returned value is further than the bound from what a bf16 plane gives."""
    check_restatement()
    n, nlist, k = 3000, 8, 50
    rows = O.generate(0x5EED0001, 2, 0, n, d)
    qall = O.generate(0x5EED0002, 2, 0, 24, d)
    ref, mag, npn = approx_reference(rows, qall, metric)
    tol = tolerance(metric, d, ref, mag, npn)
    # the same value from bf16 roundings (what a plane that is not fp8 would give)
    r16, q16 = (O.normalize(rows), O.normalize(qall)) if metric == "Cosine" else (rows, qall)
    ip16 = bf16_round(q16) @ bf16_round(r16).T
    ref16 = npn - 2 * ip16 if metric == "L2" else 1 - ip16 if metric == "Cosine" else ip16
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
    try:
        assert idx.plane()["format"] == 1
        for nq in (3, 24):
            ids, dist = idx.search(qall[:nq], k, {"nprobe": nlist}, first_stage_only=True)
            assert (ids >= 0).all() and all(len(set(r)) == k for r in ids.tolist())
            qi = np.arange(nq)[:, None]
            err = np.abs(dist.astype(np.float64) - ref[qi, ids])
            print(f"first stage d={d} {metric} nq={nq}: max err / tol {np.max(err / tol[qi, ids]):.3f}")
            assert np.all(err <= tol[qi, ids]), (metric, d, nq, np.max(err / tol[qi, ids]))
            # the k-th returned value against the reference's k-th best
            order = np.argsort(-ref[:nq] if metric == "IP" else ref[:nq], axis=1, kind="stable")
            kth = order[:, k - 1]
            # (k-th order statistics of two sequences that differ by at most t
            # per element differ by at most t: t = the query's largest tolerance)
            assert np.all(np.abs(dist[:, k - 1].astype(np.float64) - ref[np.arange(nq), kth]) <= tol[:nq].max(axis=1))
            # not bf16: the input separates the two planes, and so does the output
            sep = np.abs(ref[qi, ids] - ref16[qi, ids]) > 2 * tol[qi, ids]
            assert sep.any(), "the case's rows do not separate fp8 from bf16"
            assert (np.abs(dist.astype(np.float64) - ref16[qi, ids]) > tol[qi, ids])[sep].any()
    finally:
        idx.free()
        seg.free()


# ---- 3. exhaustive == FLAT, bit for bit, pruning on ---------------------------

EXHAUSTIVE = [
    # name,           n,     d,   nq, k,   metric,  mode, gran, nlist, filter, lwd
    ("l2_nq1",        6000,  64,  1,  10,  "L2",     2, 1024, 8,  None, None),
    ("l2_nq32",       9000,  128, 32, 50,  "L2",     2, 2048, 16, None, None),
    ("ip_nq5",        7000,  96,  5,  20,  "IP",     1, 1024, 8,  None, None),
    ("ip_nq40",       7000,  96,  40, 100, "IP",     2, 1024, 12, None, None),
    ("cos_nq3",       8000,  128, 3,  30,  "Cosine", 2, 512,  10, None, None),
    ("cos_nq64_768",  6000,  768, 64, 100, "Cosine", 2, 1024, 16, None, None),
    ("l2_filter",     8000,  64,  24, 40,  "L2",     2, 1024, 8,  0.3,  None),
    ("cos_filter_lwd", 8000, 64,  7,  40,  "Cosine", 2, 512,  8,  0.5,  0.2),
    ("ip_lwd",        8000,  48,  21, 30,  "IP",     1, 1024, 8,  None, 0.3),
    ("l2_d3_small",   300,   3,   20, 100, "L2",     0, 64,   4,  None, None),
]


@pytest.mark.parametrize("cfg", EXHAUSTIVE, ids=[c[0] for c in EXHAUSTIVE])
def test_exhaustive_equals_flat(mq, cfg):
    name, n, d, nq, k, metric, mode, gran, nlist, fsel, lwd = cfg
    rows = O.generate(0x5EED0001, mode, 0, n, d)
    q = O.generate(0x5EED0002, mode, 0, nq, d)
    rng = np.random.default_rng(n + nq)
    fbits = rng.random(n) < fsel if fsel else np.ones(n, bool)
    ebits = rng.random(n) >= lwd if lwd else np.ones(n, bool)
    flt = np.packbits(fbits.astype(np.uint8), bitorder="little") if fsel else None
    ex = np.packbits(ebits.astype(np.uint8), bitorder="little") if lwd else None
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
    try:
        info = idx.info()
        assert info["nlist"] == nlist and info["rows_indexed"] == n and idx.plane()["format"] == 1
        flat = seg.search(q, k, filter_bitmap=flt, row_exists=ex)
        # the input, before the kernel: every exact top-k row is among the
        # 4096 best fp8 values of its query
        valid = fbits & ebits
        if valid.sum() > 4096:
            ref, _, _ = approx_reference(rows, q, metric)
            key = np.where(valid[None, :], ref if metric != "IP" else -ref, np.inf)
            rank = np.argsort(np.argsort(key, axis=1, kind="stable"), axis=1)
            worst = max(rank[i, r] for i in range(nq) for r in flat[0][i] if r >= 0)
            assert worst < 4096, (name, worst)
        got = idx.search(q, k, {"nprobe": nlist, "num_reorder": 4096}, filter_bitmap=flt, row_exists=ex)
        st = mq.vector_index.last_index_stats()
    finally:
        idx.free()
        seg.free()
    assert st["nprobe"] == nlist and st["num_reorder"] == 4096
    same_bits(got, flat, name)


# ---- 4. pair mode and ragged lists -------------------------------------------

def _check_against_rerank(mq, seg, idx, q, k, nprobe, ctx):
    """ids from the probed lists only, exact distances in the reference
    order, and the pruned search == re-ranking every candidate."""
    params = {"nprobe": nprobe}
    got = idx.search(q, k, params)
    full = idx.search(q, k, params, rerank_all=True)
    same_bits(got, full, f"{ctx} pruned vs rerank_all")
    off, lrows = idx.lists()
    pr = idx.probes(q, params)
    for i in range(len(q)):
        members = np.concatenate([lrows[off[l]:off[l + 1]] for l in pr[i] if l >= 0])
        members = members[members >= 0]
        found = got[0][i][got[0][i] >= 0]
        assert np.isin(found, members).all(), ctx
        assert len(found) == min(k, len(members)), ctx
    same_bits(seg.rerank(q, got[0], k), got, f"{ctx} vs rerank")


RAGGED = [(1, 1), (1, 3), (4, 1), (4, 3), (64, 3)]  # 16 nq nprobe <= 64 lists: pair mode, else the grouped plan


@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_pair_and_grouped_mode(mq, metric):
    n, d, nlist, k = 5000, 64, 64, 10
    seg = mq.VectorScanSegment.generate(0x5EED0001, 2, n, d, metric=metric, granule=1024)
    q = O.generate(0x5EED0001, 2, n, 64, d)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
    try:
        for nq, nprobe in RAGGED:
            _check_against_rerank(mq, seg, idx, q[:nq], k, nprobe, f"{metric} nq {nq} nprobe {nprobe}")
            idx.search(q[:nq], k, {"nprobe": nprobe})
            st = mq.vector_index.last_index_stats()
            assert st["pairs"] == nq * nprobe and st["values"] > 0, st
            if 16 * nq * nprobe <= nlist:  # pair mode reads a list once per pair: 1 B per element
                assert st["plane_bytes"] == st["values"] * 64, st
    finally:
        idx.free()
        seg.free()


def test_empty_and_short_lists(mq):
    """40 distinct rows, five copies of each, 64 lists: centroids that start
    as copies of one another lose every tie to the first, so some lists are
    empty and the others hold fewer than 16 rows."""
    d, k = 64, 10
    base = O.generate(0x5EED0003, 1, 0, 40, d)
    rows = np.repeat(base, 5, axis=0)
    q = O.generate(0x5EED0004, 1, 0, 24, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=64)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 64, "plane": "fp8"})
    try:
        off, lrows = idx.lists()
        count = np.array([(lrows[off[l]:off[l + 1]] >= 0).sum() for l in range(64)])
        assert (count == 0).any() and ((count > 0) & (count < 16)).any() and count.sum() == 200, count
        for nq, nprobe in ((1, 1), (4, 3), (24, 8), (24, 64)):
            _check_against_rerank(mq, seg, idx, q[:nq], k, nprobe, f"short lists nq {nq} nprobe {nprobe}")
        same_bits(idx.search(q, k, {"nprobe": 64, "num_reorder": 4096}), seg.search(q, k), "short lists, every list")
    finally:
        idx.free()
        seg.free()


def test_list_longer_than_a_work_item(mq):
    n, d, k = 3000, 64, 10
    seg = mq.VectorScanSegment.generate(0x5EED0001, 2, n, d, metric="IP", granule=1024)
    q = O.generate(0x5EED0001, 2, n, 24, d)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 2, "plane": "fp8"})
    try:
        assert idx.info()["max_list"] > 512
        for nq, nprobe in ((1, 1), (1, 2), (24, 1), (24, 2)):
            _check_against_rerank(mq, seg, idx, q[:nq], k, nprobe, f"long list nq {nq} nprobe {nprobe}")
        same_bits(idx.search(q, k, {"nprobe": 2, "num_reorder": 4096}), seg.search(q, k), "long lists, every list")
    finally:
        idx.free()
        seg.free()


# ---- 5. value classes ----------------------------------------------------------

@pytest.fixture(scope="module")
def segs(mq):
    """(class, metric) -> its resident segment, built on first use."""
    cache = {}

    def get(name, metric):
        if (name, metric) not in cache:
            c = V.case(name)
            cache[name, metric] = mq.VectorScanSegment.from_rows(c.rows, metric=metric, granule=c.granule)
        return cache[name, metric]

    yield get
    for seg in cache.values():
        seg.free()


INDEXED = [(n, m) for n in ("big17", "tiny20", "cut", "negip", "qspecial_base", "specials") for m in V.ALL]


@pytest.mark.parametrize("name,metric", INDEXED, ids=[f"{n}-{m}" for n, m in INDEXED])
def test_value_classes_exhaustive_equals_flat(mq, segs, name, metric):
    """The default index with an fp8 plane, every list probed and every row
    re-ranked (num_reorder 4096 >= n), returns FLAT's result, which equals the
    oracle's: rows of magnitude 1e17 and 1e-20 (scale exponents far from
    zero; the product of two scales outside the fp32 range), NaN, infinite
    and denormal rows (NaN codes, scale exponent 0 or 156), special queries."""
    c = V.case(name)
    n = c.rows.shape[0]
    seg = segs(name, metric)
    idx = mq.VectorIndex.build(seg, "MSTG", FP8)
    try:
        info = idx.info()
        assert info["rows_indexed"] == n and info["nlist"] > 1 and idx.plane()["format"] == 1, info
        params = {"nprobe": info["nlist"], "num_reorder": 4096}
        for nq in (4, 64):
            q = c.queries[:nq]
            got = idx.search(q, c.k, params)
            st = mq.vector_index.last_index_stats()
            assert st["nprobe"] == info["nlist"] and st["num_reorder"] == 4096, st
            flat = seg.search(q, c.k)
            same_bits(got, flat, f"index {name} {metric} nq={nq}")
            same_bits(flat, V.reference(name, metric, nq), f"flat {name} {metric} nq={nq}")
    finally:
        idx.free()


# name, metric, k, num_reorder, whether every candidate must be re-ranked
PRUNED = [
    ("cut", "IP", 1000, 1500, True),
    ("negip", "IP", 1200, 1400, True),
    ("qspecial_base", "IP", 50, 200, False),
    ("qspecial_base", "L2", 50, 200, False),
    ("big17", "Cosine", 50, 200, False),
]


@pytest.mark.parametrize("name,metric,k,R,every", PRUNED, ids=[f"{p[0]}-{p[1]}" for p in PRUNED])
def test_value_classes_pruned_equals_full(mq, segs, name, metric, k, R, every):
    c = V.case(name)
    seg = segs(name, metric)
    idx = mq.VectorIndex.build(seg, "MSTG", FP8)
    try:
        params = {"nprobe": idx.info()["nlist"], "num_reorder": R}
        for nq in (4, 64):
            q = c.queries[:nq]
            full = idx.search(q, k, params, rerank_all=True)
            assert mq.vector_index.last_index_stats()["reranked"] == nq * R
            pruned = idx.search(q, k, params)
            st = mq.vector_index.last_index_stats()
            print(f"pruned {name} {metric} nq={nq}: reranked {st['reranked']} of {nq * R}")
            assert 0 < st["reranked"] <= nq * R, st
            if every:
                assert st["reranked"] == nq * R, st
            same_bits(pruned, full, f"pruned {name} {metric} nq={nq}")
    finally:
        idx.free()


# ---- 6. recall at the default parameters ----------------------------------------

@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_recall_default_params(mq, metric):
    n, d, nq, k = 60000, 128, 200, 100
    seg = mq.VectorScanSegment.generate(0x5EED0001, 2, n, d, metric=metric)
    q = O.generate(0x5EED0001, 2, n, nq, d)
    idx = mq.VectorIndex.build(seg, "MSTG", FP8)
    try:
        assert idx.plane()["format"] == 1
        ids_i, dist_i = idx.search(q, k)
        st = mq.vector_index.last_index_stats()
        ids_f, _ = seg.search(q, k)
        ids_r, dist_r = seg.rerank(q, ids_i, k)
    finally:
        idx.free()
        seg.free()
    recall = np.mean([len(set(ids_i[i, :10]) & set(ids_f[i, :10])) for i in range(nq)]) / 10
    print(f"fp8 recall@10 {metric}: {recall:.4f}, reranked {st['reranked']} of {nq * st['num_reorder']}")
    assert recall >= 0.95, recall
    same_bits((ids_r, dist_r), (ids_i, dist_i), metric)


# ---- 7. save and load -----------------------------------------------------------

def test_save_and_load(mq):
    n, d, nlist, k = 5000, 100, 37, 10
    rows = O.generate(0x5EED0101, 2, 0, n, d)
    q = O.generate(0x5EED0102, 2, 0, 24, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="Cosine", granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
    b16 = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    ld = None
    try:
        blob = idx.save()
        content = O.decompress_stream(blob, len(blob), verify=True)
        assert content[56:60] == (1).to_bytes(4, "little") and content[60:64] == b"\0" * 4
        assert parse_header(content)["reserved"] == b"\x01\0\0\0" + b"\0" * 4
        blob16 = b16.save()
        content16 = O.decompress_stream(blob16, len(blob16), verify=True)
        assert parse_header(content16)["reserved"] == b"\0" * 8
        assert content16[:56] == content[:56] and content16[64:] == content[64:]
        ld = mq.VectorIndex.load(seg, blob)
        assert ld.plane() == idx.plane() and ld.plane()["format"] == 1
        a, b = ld.info(), idx.info()
        a.pop("build_ms"), b.pop("build_ms")
        assert a == b
        for kw in ({}, {"params": {"nprobe": nlist, "num_reorder": 4096}}, {"first_stage_only": True}):
            for nq in (5, 24):
                same_bits(ld.search(q[:nq], k, **kw), idx.search(q[:nq], k, **kw), f"loaded {kw} nq {nq}")
        assert ld.save() == blob
        # an unknown plane format, block checksums recomputed by the oracle's writer
        forged = O.compress_stream(content[:56] + (7).to_bytes(4, "little") + content[60:], method=0x02)
        with pytest.raises(mq._lib.MqvsError) as e:
            mq.VectorIndex.load(seg, forged).free()
        assert e.value.status == mq._lib.ERR_ILLEGAL_COLUMN
        same_bits(ld.search(q, k), idx.search(q, k), "after the refused load")
    finally:
        for ix in (idx, b16, ld):
            if ix is not None:
                ix.free()
        seg.free()


def test_part_cache_weighs_the_smaller_plane(mq):
    """The part cache takes an fp8 index as any other and weighs the pair by
    its hbm_bytes."""
    n, d = 4000, 64
    seg = mq.VectorScanSegment.generate(0x5EED0001, 2, n, d, metric="L2")
    q = O.generate(0x5EED0001, 2, n, 8, d)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 16, "plane": "fp8"})
    expect = idx.search(q, 10)
    weight = seg.info()["hbm_bytes"] + idx.info()["hbm_bytes"]
    from myscaledb_amd.cache import PartCache
    cache = PartCache(1 << 30)
    try:
        cache.put("part", seg, idx)
        assert cache.stats()["bytes"] == weight
        s2, i2 = cache.acquire("part")
        assert i2.plane()["format"] == 1
        same_bits(i2.search(q, 10), expect, "cached fp8 index")
        cache.release("part", s2)
    finally:
        cache.free()


# ---- 8. rows in host memory ------------------------------------------------------

def test_rows_in_host_memory(mq):
    n, d, nlist, k = 4000, 100, 16, 10
    rows = O.generate(0x5EED0101, 2, 0, n, d)
    q = O.generate(0x5EED0102, 2, 0, 24, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="Cosine", granule=1024)
    try:
        idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
        expect = idx.search(q, k, {"nprobe": 4})
        lists = idx.lists()
        idx.free()
        seg.set_rows_host(True)
        assert seg.info()["rows_host"]
        idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": "fp8"})
        try:
            assert idx.plane()["format"] == 1
            for a, b in zip(idx.lists(), lists):
                assert np.array_equal(a, b)
            same_bits(idx.search(q, k, {"nprobe": 4}), expect, "rows in host memory")
        finally:
            idx.free()
    finally:
        seg.free()
