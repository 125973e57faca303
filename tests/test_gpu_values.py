"""Values outside the ordinary range (value_cases.py: NaN, infinities,
overflowing and denormal magnitudes, rows and lists that straddle a validity
cut) through every path that can serve them, HIP vs the CPU oracle, ids and
distance bits.  test_oracle_values.py keeps the classes themselves honest.

Each case asserts the path it took (last_search_stats / seg.info), so a case
cannot pass by quietly taking another one:

* a segment whose largest row norm is finite and below 1e18 keeps its bf16
  pre-filter (info: prefilter 2, approx_ok) and its searches report path 2;
  `specials` (non-finite norms) is served by the exact kernels: path 0 (VALU,
  direct formula) below 20 queries, path 1 (fp32 MFMA, BLAS formula) from 20;
* a pre-filtered search whose bound keeps more than 4096 candidates of some
  query re-runs on the exact kernels: the stats are then the re-run's (path
  0 / 1) with rescans == 1; so does one with a query of norm 1e18 or more.
  _fallback says where that happens, and why; everywhere else rescans == 0.
  qspecial's q0, q1, q3, q6 and tie_inf's q0 are such queries (NaN, +inf,
  all 1e30, five +inf): no batch that holds one can take path 2, and q0 is
  in every batch of those two classes.  Their other queries -- zeros, -0.0,
  all 1e-30, the ordinary ones -- go through the pre-filter in the classes
  qfinite_base, qfinite_big17 and tie_fin (the same parts, the query sets
  without those queries): path 2, rescans 0 at every nq.

One segment per (class, metric) is shared by the module (fixture `segs`).
"""
import numpy as np
import pytest

import value_cases as V
from oracle import oracle as O
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

NQS = (1, 4, 24, 200)  # direct formula (1 and 4), BLAS formula, batch probe (> 128 queries)
EXACT_ONLY = ("specials",)  # approx_ok false: NaN / infinite row norms


def _fallback(name, metric, nq):
    """Whether the exact kernels end up serving a search of a segment that
    has its pre-filter (stats: the re-run's path 0 / 1, rescans == 1).

    * A query whose norm is NaN, infinite or at least 1e18 (k_query_bound's
      limit, the rows' approx_ok limit on the query side): the approximate sum
      can overflow to NaN where the exact chain stays valid, so the search is
      not trusted to the bound.  qspecial's q0 (NaN) and tie_inf's q0 (+inf)
      are in every batch; under cosine the limit applies to the normalised
      query, which is NaN for both.
    * tiny20: products of two 1e-20 values are ~1e-40 and distances ~1e-39,
      far below the absolute slack 1e-30 of k_query_bound and widen (and the
      2.4e-7 of cosine's 1 - ip), so every one of the 5000 rows is within the
      bound of the k-th: more than the 4096 survivors a query may keep.
    """
    if name == "tiny20":
        return True
    with np.errstate(all="ignore"):
        norm = np.sqrt((V.case(name).queries[:nq].astype(np.float64) ** 2).sum(axis=1))
    if metric == "Cosine":
        return bool((~np.isfinite(norm)).any())
    return bool((~(norm < 1e18)).any())


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


@pytest.fixture(scope="module")
def segs(mq):
    """(class, metric) -> its resident segment, built on first use."""
    cache = {}

    def get(name, metric):
        if (name, metric) not in cache:
            c = V.case(name)
            seg = mq.VectorScanSegment.from_rows(c.rows, metric=metric, granule=c.granule)
            info = seg.info()
            assert info["prefilter"] == 2, info
            assert info["approx_ok"] == (name not in EXACT_ONLY), (name, info)
            cache[name, metric] = seg
        return cache[name, metric]

    yield get
    for seg in cache.values():
        seg.free()


def _exact_path(nq):
    return 0 if nq < 20 else 1


def _stats(ctx, approx, nq, fallback=False, gather=None):
    """The path assertions of one search that has just run."""
    from myscaledb_amd import _lib
    st = _lib.last_search_stats()
    print(ctx, {f: st[f] for f in ("path", "prefilter", "rescans", "gather", "batch_kernel", "survivors_max",
                                    "candidates_max")})
    if approx and not fallback:
        assert st["path"] == 2 and st["prefilter"] == 2 and st["rescans"] == 0, (ctx, st)
    elif approx:
        assert st["path"] == _exact_path(nq) and st["rescans"] == 1, (ctx, st)
    else:
        assert st["path"] == _exact_path(nq) and st["prefilter"] == 0 and st["rescans"] == 0, (ctx, st)
    if gather is not None:
        assert st["gather"] == gather, (ctx, st)
    return st


CM_IDS = [f"{n}-{m}" for n, m in V.CASE_METRICS]


# (nq 7: every special query of qspecial under the direct formula)
DEFAULT = [(n, m, nq) for n, m in V.CASE_METRICS for nq in NQS + ((7,) if n.startswith("qspecial") else ())]


@pytest.mark.parametrize("name,metric,nq", DEFAULT, ids=[f"{n}-{m}-nq{q}" for n, m, q in DEFAULT])
def test_default_path(segs, name, metric, nq):
    c = V.case(name)
    ids_o, dist_o = V.reference(name, metric, nq)
    ctx = f"default {name} {metric} nq={nq}"
    ids, dist = segs(name, metric).search(c.queries[:nq], c.k)
    assert_bitwise(ids, dist, ids_o, dist_o, ctx)
    st = _stats(ctx, name not in EXACT_ONLY, nq, _fallback(name, metric, nq))
    if nq > 128 and name not in EXACT_ONLY and not _fallback(name, metric, nq):
        # 1500 .. 6000 rows are a dense probe of every row: the batch kernel
        # has no main scan to run, its probe kernel k_scan_hi<2,4,4> decides
        assert st["main_rows"] == 0 and st["batch_kernel"] == 0, (ctx, st)


@pytest.mark.parametrize("nq", (4, 24))
@pytest.mark.parametrize("name,metric", V.CASE_METRICS, ids=CM_IDS)
def test_exact_flag_and_batch_mode(segs, name, metric, nq):
    """exact=True and set_batch_mode(1): the exact kernels over a segment
    that has its planes."""
    from myscaledb_amd.vector_scan import set_batch_mode
    c = V.case(name)
    ids_o, dist_o = V.reference(name, metric, nq)
    seg = segs(name, metric)
    ids, dist = seg.search(c.queries[:nq], c.k, exact=True)
    _stats(f"exact flag {name} {metric} nq={nq}", False, nq)
    assert_bitwise(ids, dist, ids_o, dist_o, f"exact flag {name} {metric} nq={nq}")
    set_batch_mode(1)
    try:
        ids, dist = seg.search(c.queries[:nq], c.k)
        _stats(f"batch mode 1 {name} {metric} nq={nq}", False, nq)
    finally:
        set_batch_mode(0)
    assert_bitwise(ids, dist, ids_o, dist_o, f"batch mode 1 {name} {metric} nq={nq}")


@pytest.mark.parametrize("name,metric", V.CASE_METRICS, ids=CM_IDS)
def test_segment_without_planes(mq, name, metric):
    """A segment built under set_prefilter(0): path 0 at nq 4, 1 at nq 24."""
    from myscaledb_amd.vector_scan import set_prefilter
    c = V.case(name)
    set_prefilter(0)
    try:
        seg = mq.VectorScanSegment.from_rows(c.rows, metric=metric, granule=c.granule)
    finally:
        set_prefilter(2)
    try:
        info = seg.info()
        assert info["prefilter"] == 0 and not info["approx_ok"], info
        for nq in (4, 24):
            ids, dist = seg.search(c.queries[:nq], c.k)
            _stats(f"no planes {name} {metric} nq={nq}", False, nq)
            assert_bitwise(ids, dist, *V.reference(name, metric, nq), f"no planes {name} {metric} nq={nq}")
    finally:
        seg.free()


@pytest.mark.parametrize("name,metric", [("tiny20", "L2"), ("cut", "IP"), ("eps_plus", "Cosine")])
def test_rows_in_host_memory(mq, name, metric):
    """set_rows_host(True): the pre-filter reads the bf16 plane in HBM, the
    exact re-rank reads the fp32 rows over PCIe."""
    c = V.case(name)
    seg = mq.VectorScanSegment.from_rows(c.rows, metric=metric, granule=c.granule)
    try:
        seg.set_rows_host(True)
        info = seg.info()
        assert info["rows_host"] and info["approx_ok"] and info["prefilter"] == 2, info
        for nq in (4, 24):
            ids, dist = seg.search(c.queries[:nq], c.k)
            _stats(f"host rows {name} {metric} nq={nq}", True, nq, _fallback(name, metric, nq))
            assert_bitwise(ids, dist, *V.reference(name, metric, nq), f"host rows {name} {metric} nq={nq}")
    finally:
        seg.free()


def _bitmaps(name, granule):
    """50 % PREWHERE filter with the second granule cleared whole (a skipped
    chunk: later chunks' cosine ordinals shift) + 10 % deletes."""
    n = V.case(name).rows.shape[0]
    rs = np.random.RandomState(0xF117 + n)
    flt = rs.random_sample(n) < 0.5
    whole = flt.copy()
    flt[granule:2 * granule] = False
    ex = rs.random_sample(n) >= 0.1
    return [np.packbits(b, bitorder="little") for b in (flt, ex, whole)]


FILTERED = [(n, m) for n in ("specials", "cut") for m in ("IP", "Cosine")]


@pytest.mark.parametrize("gather", (False, True))
@pytest.mark.parametrize("name,metric", FILTERED, ids=[f"{n}-{m}" for n, m in FILTERED])
def test_filter_and_deletes(segs, name, metric, gather):
    c = V.case(name)
    flt, ex, whole = _bitmaps(name, c.granule)
    g = c.granule
    seg = segs(name, metric)
    approx = name not in EXACT_ONLY
    for nq in (4, 24):
        ctx = f"filter {name} {metric} nq={nq} gather={gather}"
        ids_o, dist_o = O.vector_scan(c.rows, c.queries[:nq], c.k, O.METRICS[metric], c.granule, filter_bits=flt,
                                      row_exists_bits=ex, fast=True)
        ids, dist = seg.search(c.queries[:nq], c.k, filter_bitmap=flt, row_exists=ex, gather=gather)
        # (the fp32 MFMA kernel has no gathered form: forced gathering applies
        # to the pre-filter and to the VALU kernel)
        _stats(ctx, approx, nq, gather=int(gather and (approx or nq < 20)))
        assert_bitwise(ids, dist, ids_o, dist_o, ctx)
        # the case is not hollow: with the second granule left in the filter
        # its rows are among the results, without it none is, and results
        # come from the chunks after it (cosine: their ordinals moved up)
        ids_w, _ = O.vector_scan(c.rows, c.queries[:nq], c.k, O.METRICS[metric], g, filter_bits=whole,
                                 row_exists_bits=ex, fast=True)
        assert ((ids_w >= g) & (ids_w < 2 * g)).any(axis=1).sum() >= nq // 2, ctx
        assert not ((ids_o >= g) & (ids_o < 2 * g)).any(), ctx
        assert (ids_o >= 2 * g).any(axis=1).sum() >= nq // 2, ctx


RERANKED = [(n, m) for n in ("specials", "cut", "tie_inf") for m in V.ALL]


@pytest.mark.parametrize("name,metric", RERANKED, ids=[f"{n}-{m}" for n, m in RERANKED])
def test_rerank_of_every_row_equals_search(segs, name, metric):
    """mqvs_rerank with every row as a candidate (6000 of tie_inf: sorted
    through global scratch) returns the search's result."""
    c = V.case(name)
    n = c.rows.shape[0]
    seg = segs(name, metric)
    for nq in (4, 24):
        cand = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
        ids, dist = seg.rerank(c.queries[:nq], cand, c.k)
        assert_bitwise(ids, dist, *V.reference(name, metric, nq), f"rerank {name} {metric} nq={nq}")


@pytest.mark.parametrize("metric", ("L2", "IP"))
@pytest.mark.parametrize("name", ("specials", "negip"))
def test_try_brute_force_search(mq, name, metric):
    """mqvs_knn_raw against faiss's knn: raw IP keeps every ip > -FLT_MAX
    (negative values, -FLT_MAX padding), unlike the operator."""
    c = V.case(name)
    n, d = c.rows.shape
    for nq in (4, 24):
        ids_o, dist_o = O.knn(c.queries[:nq], c.rows, c.k, O.METRICS[metric], fast=True)
        ids, dist = mq.try_brute_force_search(c.queries[:nq], c.rows, d, c.k, nq, n, metric)
        _stats(f"knn {name} {metric} nq={nq}", name not in EXACT_ONLY, nq)
        assert_bitwise(ids.reshape(nq, c.k), dist.reshape(nq, c.k), ids_o, dist_o, f"knn {name} {metric} nq={nq}")
        if metric == "IP" and name == "negip":
            assert (dist_o < 0).any()


@pytest.mark.parametrize("metric", V.ALL)
@pytest.mark.parametrize("name", ("specials", "negip"))
def test_merge_of_two_shards(mq, name, metric):
    """Two row-range shards + mqvs_merge_shards == the one-part search: IP
    lists that end in (-1, FLT_MIN) padding, lists holding +inf."""
    c = V.case(name)
    n = c.rows.shape[0]
    cut = 3 * c.granule
    shards = [mq.VectorScanSegment.from_rows(c.rows[a:b], metric=metric, granule=c.granule, row_offset=a)
              for a, b in ((0, cut), (cut, n))]
    try:
        for nq in (4, 24):
            parts = []
            for seg in shards:
                parts.append(seg.search(c.queries[:nq], c.k))
                _stats(f"shard {name} {metric} nq={nq}", name not in EXACT_ONLY, nq)
            mi, md = mq.merge_shards(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), metric)
            assert_bitwise(mi, md, *V.reference(name, metric, nq), f"merge {name} {metric} nq={nq}")
    finally:
        for seg in shards:
            seg.free()


def test_ingest_keeps_every_bit_pattern(mq):
    """from_column over the specials' bit patterns + a signalling NaN, NaNs
    with payloads and the extreme denormals: the resident rows are the same
    words, and a search equals the oracle on them."""
    from test_gpu_ingest import column_files, device_rows
    c = V.case("specials")
    n, d = c.rows.shape
    words = c.rows.view(np.uint32).copy()
    extra = [0x7FA00000, 0x7FC12345, 0xFFC00001, 0xFF800001, 0x007FFFFF, 0x00000001, 0x807FFFFF, 0x80000001]
    for i, w in enumerate(extra):
        words[17 + 301 * i, (5 * i) % d] = w
    rows = words.view(np.float32)
    db, sb = column_files(rows, np.full(n, d, np.uint64), block=65536)
    seg = mq.VectorScanSegment.from_column(db, sb, n, d, metric="L2", granule=c.granule)
    try:
        assert np.array_equal(device_rows(mq, seg).view(np.uint32), words)
        for nq in (4, 24):
            ids, dist = seg.search(c.queries[:nq], c.k)
            _stats(f"ingest nq={nq}", False, nq)
            ids_o, dist_o = O.vector_scan(rows, c.queries[:nq], c.k, O.L2, c.granule, fast=True)
            assert_bitwise(ids, dist, ids_o, dist_o, f"ingest nq={nq}")
    finally:
        seg.free()


def _same_bits(a, b, ctx):
    assert_bitwise(a[0], a[1], b[0], b[1], ctx)


INDEXED = [(n, m) for n in ("big17", "tiny20", "cut", "negip", "qspecial_base", "specials") for m in V.ALL]


@pytest.mark.parametrize("name,metric", INDEXED, ids=[f"{n}-{m}" for n, m in INDEXED])
def test_index_exhaustive_equals_flat(mq, segs, name, metric):
    """The default index, every list probed and every row re-ranked
    (num_reorder 4096 >= n), returns FLAT's result -- which the tests above
    pin to the oracle.  cut / negip (IP lists that end under the FLT_MIN cut)
    and qspecial (NaN and infinite bounds) are the cases in which the
    re-rank's pruning must stay off (wave_prune_cut).

    specials: a row with a NaN component has a NaN distance to every centroid
    and the k-means assignment (a FLAT top-1 search over the centroids)
    returns -1 for it, as for an infinite row whose products with every
    centroid are -inf or NaN; the build files those rows under list 0, so
    every row is in a list (rows_indexed == n).  The list numbers come from
    that search's ids alone (host integers checked against [0, nlist)), the
    centroid means from the grouped rows: a NaN can reach a centroid's value,
    never an index."""
    c = V.case(name)
    n = c.rows.shape[0]
    seg = segs(name, metric)
    idx = mq.VectorIndex.build(seg)
    try:
        info = idx.info()
        assert info["rows_indexed"] == n and info["nlist"] > 1, info
        params = {"nprobe": info["nlist"], "num_reorder": 4096}
        for nq in (4, 64):
            q = c.queries[:nq]
            got = idx.search(q, c.k, params)
            st = mq.vector_index.last_index_stats()
            assert st["nprobe"] == info["nlist"] and st["num_reorder"] == 4096, st
            flat = seg.search(q, c.k)
            _same_bits(got, flat, f"index {name} {metric} nq={nq}")
            _same_bits(flat, V.reference(name, metric, nq), f"flat {name} {metric} nq={nq}")
    finally:
        idx.free()


# name, metric, k, num_reorder, whether every candidate must be re-ranked
PRUNED = [
    # IP lists that end under the FLT_MIN cut inside k: the k-th approximate
    # value less the bound is not above FLT_MIN (cut: the bound's absolute
    # slack 1e-30 alone exceeds every value; negip: the 1200th value is
    # negative), so wave_prune_cut must refuse to prune
    ("cut", "IP", 1000, 1500, True),
    ("negip", "IP", 1200, 1400, True),
    ("qspecial_base", "IP", 50, 200, False),
    ("qspecial_base", "L2", 50, 200, False),
    ("big17", "Cosine", 50, 200, False),
]


@pytest.mark.parametrize("name,metric,k,R,every", PRUNED, ids=[f"{p[0]}-{p[1]}" for p in PRUNED])
def test_index_pruned_rerank_equals_full(mq, segs, name, metric, k, R, every):
    """num_reorder below n with the bound pruning on (the default) returns
    the bits of re-ranking every candidate (rerank_all); where the k best can
    fall under the IP cut the pruned search re-ranks every candidate too.
    (qspecial: per query, a NaN or infinite bound or a NaN candidate turns
    pruning off; the stats count candidates over the batch, so only the bits
    are compared there.)"""
    c = V.case(name)
    seg = segs(name, metric)
    idx = mq.VectorIndex.build(seg)
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
            _same_bits(pruned, full, f"pruned {name} {metric} nq={nq}")
    finally:
        idx.free()


def test_async_search_with_an_unbounded_query_is_reported(mq, segs):
    """An ASYNC search cannot re-run itself: a batch that holds a query the
    bound does not cover (norm NaN, infinite or >= 1e18) is reported by
    mqvs_async_check, naming that cause, and the check is cleared; the same
    batch without such queries checks clean and equals the synchronous
    result."""
    import torch
    from myscaledb_amd._lib import MqvsError
    from myscaledb_amd.vector_scan import async_check
    seg = segs("qspecial_base", "IP")
    k = V.case("qspecial_base").k
    for which in ([0], [1], [3]):  # NaN, +inf, all 1e30
        q = torch.from_numpy(V.case("qspecial_base").queries[which + list(range(7, 30))].copy()).cuda()
        seg.search(q, k, async_=True)
        with pytest.raises(MqvsError, match="norm is NaN, infinite or at least 1e18") as e:
            async_check()
        assert e.value.name == "LOGICAL_ERROR"
        async_check()  # cleared
    q = torch.from_numpy(V.case("qfinite_base").queries[:24].copy()).cuda()
    ids, dist = seg.search(q, k, async_=True)
    async_check()
    assert_bitwise(ids.cpu().numpy(), dist.cpu().numpy(), *V.reference("qfinite_base", "IP", 24), "async qfinite")
