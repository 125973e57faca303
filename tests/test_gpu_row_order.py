"""FLAT searches of parts whose rows are ordered by distance to the queries
(row_order_cases.py), against the CPU oracle bit for bit.

On a part that drifts towards the queries the probe's threshold is loose for
every later row, so a main-scan segment appends almost all of its rows: with
more rows in a segment than a candidate list holds (capacity
min(2^20, 2^25 / nq) per query, cand_capacity in search_host.h) the lists
overflow with no tie anywhere, the bf16 route falls back to the exact one, and
the exact route and the binary search re-scan the part (rescan_on_overflow,
workspace.h).  The overflow cases below reach that on every scan kernel; each
checks with numpy, from the search's own probe length, that a segment of the
plan really holds more passing rows than the capacity -- a later tuning change
cannot quietly turn the case into one that no longer overflows.  An MqvsError
fails a case: the input has no mass tie (test_row_order_cases.py), so an
overflow error on it would be a bug.

The parity-only cases run the same data where no list can overflow (nq <= 32:
capacity 2^20 >= n) through the small-batch kernels, and the orders where the
probe already holds nearly the best rows (best_first) or sees a whole period
(sawtooth).

The placement cases pin the threshold selects that keep each thread's 4
smallest keys (kept_kth_bound, k_probe_select_wide) when one thread owns all
of the k best positions.

Every case prints the search's stats (path, rescans, segments, probe_rows,
candidates_max); rescans = r means r + 1 scans of the whole part.
"""
import zlib
from functools import lru_cache

import numpy as np
import pytest

import row_order_cases as R
from oracle import oracle as O
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

N, D, K, GRAN = 262144, 16, 10, 8192
MIN_SEG = 65536  # kMinSegRows (search.hip): no float main segment is shorter


def cand_cap(nq):
    """cand_capacity(nq, k) of search_host.h for k <= 4096, restated."""
    return min(2**20, 2**25 // nq) // 256 * 256


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def stats(ctx):
    from myscaledb_amd import _lib
    st = _lib.last_search_stats()
    print(ctx, {f: st[f] for f in ("path", "rescans", "segments", "probe_rows", "candidates_max", "gather",
                                   "batch_kernel")})
    return st


@lru_cache(maxsize=None)
def masks(n, tag):
    """(filter bitmap, row_exists bitmap, valid rows) of a case."""
    rng = np.random.default_rng(zlib.crc32(f"row_order_{tag}_{n}".encode()))
    if tag == "none":
        return None, None, np.ones(n, bool)
    if tag == "masked":  # 40 % pass the filter, 10 % deleted
        f, e = rng.random(n) < 0.4, rng.random(n) >= 0.1
        return R_pack(f), R_pack(e), f & e
    if tag == "gathered":  # 50 % pass
        f = rng.random(n) < 0.5
        return R_pack(f), None, f
    raise KeyError(tag)


def R_pack(mask):
    return np.packbits(np.asarray(mask, np.uint8), bitorder="little")


@lru_cache(maxsize=None)
def reference(metric, n, d, order, k, nq, tag="none"):
    """The oracle's result for a batch of nq queries: at nq >= 32 the result
    of the 32 distinct queries, tiled (row_order_cases.py says why that is the
    batch's result); below, the run of queries[:nq]."""
    tr = R.trend(metric, n, d, order)
    flt, rex, _ = masks(n, tag)
    q = tr.queries[:min(nq, R.NQ_DISTINCT)]
    ids, dist = O.vector_scan(tr.rows, q, k, O.METRICS[metric], GRAN, filter_bits=flt, row_exists_bits=rex, fast=True)
    if nq > R.NQ_DISTINCT:
        ids, dist = R.tile(ids, nq), R.tile(dist, nq)
    ids.setflags(write=False)
    dist.setflags(write=False)
    return ids, dist


def batch(tr, nq):
    return R.tile(tr.queries, nq) if nq > R.NQ_DISTINCT else np.ascontiguousarray(tr.queries[:nq])


def search_trend(mq, metric, n, d, order, nq, k, tag="none", **kw):
    """One search of the trend part -> (ids, dist, stats)."""
    tr = R.trend(metric, n, d, order)
    flt, rex, _ = masks(n, tag)
    seg = mq.VectorScanSegment.from_rows(tr.rows, metric=metric, granule=GRAN)
    try:
        ids, dist = seg.search(batch(tr, nq), k, metric, flt, rex, **kw)
        st = stats(f"{metric} n={n} d={d} {order} nq={nq} k={k} {tag} {kw}")
    finally:
        seg.free()
    return ids, dist, st


def passing_rows(metric, n, d, tag, b, e, k):
    """Per distinct query: the valid rows of [b, e) at or under the k-th best
    valid row of [0, b) (fp64).  The search's own threshold there is never
    tighter: it is a bound on that k-th value (3 radix passes, the threads'
    kept keys), widened on the bf16 route."""
    tr = R.trend(metric, n, d, "worst_first")
    valid = masks(n, tag)[2]
    dist = R.distances(metric, tr.rows[:e], tr.queries)
    head = dist[:, :b][:, valid[:b]]
    kth = np.partition(head, k - 1, axis=1)[:, k - 1]
    return (dist[:, b:e][:, valid[b:e]] <= kth[:, None]).sum(axis=1)


def check_parity(ids, dist, metric, n, d, order, k, nq, tag, ctx):
    ids_o, dist_o = reference(metric, n, d, order, k, nq, tag)
    assert_bitwise(ids, dist, ids_o, dist_o, ctx)


# ---- float routes: overflow ---------------------------------------------------

@pytest.mark.parametrize("exact", [False, True], ids=["batch_kernel", "fp32_mfma"])
@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_overflow_nq1024(mq, metric, exact):
    """nq 1024 (capacity 32768): the batch kernel k_scan_p4m, its exact
    fallback and the re-scans; with exact=True the fp32 MFMA scan
    k_scan_mfma and the re-scans.  The first main segment [P, P + 65536)
    holds more passing rows than the capacity."""
    nq = 1024
    ids, dist, st = search_trend(mq, metric, N, D, "worst_first", nq, K, exact=exact)
    P = st["probe_rows"]
    got = passing_rows(metric, N, D, "none", P, P + MIN_SEG, K)
    print("passing rows of the first main segment:", got.min(), "capacity", cand_cap(nq))
    assert got.min() > cand_cap(nq), (P, got.min())
    check_parity(ids, dist, metric, N, D, "worst_first", K, nq, "none", f"overflow {metric} exact={exact}")


@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_overflow_masked_filter_and_deletes(mq, metric):
    """A filter that passes 40 % of 524288 rows and 10 % deleted, masked scan
    (gather=False): 36 % of the scanned rows are valid, so the first main
    segment (65536 rows) cannot fill a list of 32768 and the second one
    (twice as long: growth 2 at nq >= 256) overflows it."""
    n, nq = 2 * N, 1024
    ids, dist, st = search_trend(mq, metric, n, D, "worst_first", nq, K, "masked", gather=False)
    b = st["probe_rows"] + MIN_SEG
    got = passing_rows(metric, n, D, "masked", b, b + 2 * MIN_SEG, K)
    print("passing rows of the second main segment:", got.min(), "capacity", cand_cap(nq))
    assert st["gather"] == 0, st
    assert got.min() > cand_cap(nq), (b, got.min())
    check_parity(ids, dist, metric, n, D, "worst_first", K, nq, "masked", f"masked overflow {metric}")


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_overflow_gathered(mq, metric):
    """gather=True, 50 % of 524288 rows pass: the pre-filter scan walks the
    list of the passing rows, so its probe (16384 positions: a sixteenth of
    the list) and its segments count list positions, and its first main
    segment overflows.  A batch gathers only on that route: the stats are
    then those of the exact fallback, a masked scan of all rows (half of them
    valid), whose second main segment overflows."""
    n, nq = 2 * N, 1024
    ids, dist, st = search_trend(mq, metric, n, D, "worst_first", nq, K, "gathered", gather=True)
    rows_of = np.flatnonzero(masks(n, "gathered")[2])
    got = passing_rows(metric, n, D, "gathered", rows_of[16384], rows_of[16384 + MIN_SEG], K)
    print("passing rows of the gathered scan's first main segment:", got.min(), "capacity", cand_cap(nq))
    assert got.min() > cand_cap(nq), got.min()
    P = st["probe_rows"]
    if st["gather"]:
        assert P == 16384, st
    else:
        got = passing_rows(metric, n, D, "gathered", P + MIN_SEG, P + 3 * MIN_SEG, K)
        print("passing rows of the masked scan's second main segment:", got.min())
        assert got.min() > cand_cap(nq), (P, got.min())
    check_parity(ids, dist, metric, n, D, "worst_first", K, nq, "gathered", f"gathered overflow {metric}")


def test_overflow_scan_hi(mq):
    """nq 128 (capacity 262144) is served by k_scan_hi; 720896 rows x 8: the
    main segments grow 4x (65536, 262144, the rest), and the third one,
    [P + 327680, n), holds more passing rows than the capacity."""
    n, d, nq = 720896, 8, 128
    ids, dist, st = search_trend(mq, "L2", n, d, "worst_first", nq, K)
    b = st["probe_rows"] + 5 * MIN_SEG
    got = passing_rows("L2", n, d, "none", b, n, K)
    print("passing rows of the third main segment:", got.min(), "capacity", cand_cap(nq))
    assert got.min() > cand_cap(nq), (b, got.min())
    check_parity(ids, dist, "L2", n, d, "worst_first", K, nq, "none", "k_scan_hi overflow")


def test_overflow_large_k(mq):
    """k 5000 (above the LDS sort: the final select sorts through global
    scratch, the refinements take the 3-pass radix bound), nq 512: the
    capacity is the larger of 16 k and the batch's share, max(80000, 65536)
    in whole 256s = 79872.  The probe is k n / 16384 rows and the first main
    segment two probe lengths (nq >= 256): [P, 3 P) holds more passing rows
    than the capacity.  The pre-filter route, its exact fallback and the
    segmented re-scan all run at large k."""
    k, nq = 5000, 512
    cap = max(cand_cap(nq), 16 * k) // 256 * 256
    assert cap == 79872
    ids, dist, st = search_trend(mq, "L2", N, D, "worst_first", nq, k)
    P = st["probe_rows"]
    got = passing_rows("L2", N, D, "none", P, min(N, 3 * P), k)
    print("passing rows of the first main segment:", got.min(), "capacity", cap)
    assert got.min() > cap, (P, got.min())
    check_parity(ids, dist, "L2", N, D, "worst_first", k, nq, "none", "large k overflow")


def test_large_k_ordered(mq):
    """k 5000, nq 40.  Parity only: the capacity of a large-k search is the
    larger of 16 k and the batch's share of the budget (cand_capacity), here
    838656 -- more than the part's 262144 rows, so no list can overflow."""
    k, nq = 5000, 40
    assert max(cand_cap(nq), 16 * k) > N
    ids, dist, _ = search_trend(mq, "L2", N, D, "worst_first", nq, k)
    check_parity(ids, dist, "L2", N, D, "worst_first", k, nq, "none", "large k")


# ---- float routes: parity only ------------------------------------------------

SMALL = [(nq, True) for nq in (1, 8, 19)] + [(nq, False) for nq in (1, 16, 32)]


@pytest.mark.parametrize("nq,exact", SMALL, ids=[f"nq{nq}{'_exact' if x else ''}" for nq, x in SMALL])
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_small_batches_on_ordered_rows(mq, metric, order, nq, exact):
    assert cand_cap(nq) >= N  # (no overflow possible)
    ids, dist, _ = search_trend(mq, metric, N, D, order, nq, K, exact=exact)
    check_parity(ids, dist, metric, N, D, order, K, nq, "none", f"{metric} {order} nq={nq} exact={exact}")


@pytest.mark.parametrize("order", ["best_first", "sawtooth"])
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_nq1024_other_orders(mq, metric, order):
    ids, dist, _ = search_trend(mq, metric, N, D, order, 1024, K)
    check_parity(ids, dist, metric, N, D, order, K, 1024, "none", f"{metric} {order} nq=1024")


# ---- ASYNC ----------------------------------------------------------------------

def test_async_overflow_on_ordered_rows_is_reported(mq):
    """ASYNC cannot run the host fallbacks: the L2 overflow case must leave
    LOGICAL_ERROR (49) for async_check -- overflow on tie-free data is
    reported, never silent -- and the synchronous search of the same tensors
    equals the oracle."""
    import torch
    from myscaledb_amd._lib import MqvsError
    from myscaledb_amd.vector_scan import async_check
    nq = 1024
    tr = R.trend("L2", N, D, "worst_first")
    rows = torch.from_numpy(tr.rows.copy()).cuda()
    q = torch.from_numpy(batch(tr, nq)).cuda()
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=GRAN)
    try:
        seg.search(q, K, async_=True)
        with pytest.raises(MqvsError) as e:
            async_check()
        assert e.value.code == 49
        async_check()  # cleared
        ids, dist = seg.search(q, K)
        stats("L2 device tensors, synchronous after ASYNC")
        ids, dist = ids.cpu().numpy(), dist.cpu().numpy()
    finally:
        seg.free()
    check_parity(ids, dist, "L2", N, D, "worst_first", K, nq, "none", "sync after async")


# ---- mass ties stay as they are ---------------------------------------------------

def test_mass_tie_is_the_oracle_or_an_error(mq):
    """600000 identical rows x 8, nq 64, k 10 (capacity 524288 < n): every
    row ties at the k-th distance.  Either the oracle's bits (rows 0 .. 9) or
    LOGICAL_ERROR, never another result.

    Observed: LOGICAL_ERROR ("candidate overflow: more than 524288 rows tie
    at the k-th distance"), before and after the segmented re-scan."""
    from myscaledb_amd._lib import MqvsError
    n, d, nq = 600_000, 8, 64
    rows = np.ones((n, d), np.float32)
    q = np.zeros((nq, d), np.float32)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=GRAN)
    try:
        try:
            ids, dist = seg.search(q, K)
        except MqvsError as e:
            print("mass tie:", e)
            assert e.code == 49
            return
        stats("mass tie")
    finally:
        seg.free()
    ids_o, dist_o = O.vector_scan(rows, q[:R.NQ_DISTINCT], K, O.L2, GRAN, fast=True)
    assert_bitwise(ids, dist, R.tile(ids_o, nq), R.tile(dist_o, nq), "mass tie")


# ---- binary routes ------------------------------------------------------------------

NB = 200000
BIN_WINDOW = 131072


@lru_cache(maxsize=None)
def reference_binary(metric, nbits, order, nq):
    tr = R.trend_codes(NB, nbits, order)
    ids, dist = O.vector_scan_binary(tr.rows, tr.queries[:min(nq, R.NQ_DISTINCT)], K, O.METRICS[metric], GRAN)
    if nq > R.NQ_DISTINCT:
        ids, dist = R.tile(ids, nq), R.tile(dist, nq)
    return ids, dist


def search_codes(mq, metric, nbits, order, nq, batch_min=0):
    from myscaledb_amd.vector_scan import set_binary_batch
    tr = R.trend_codes(NB, nbits, order)
    seg = mq.BinaryVectorScanSegment.from_codes(tr.rows, metric=metric)
    prev = set_binary_batch(batch_min)
    try:
        ids, dist = seg.search(batch(tr, nq), K, metric)
        st = stats(f"{metric} {nbits} bits {order} nq={nq} batch_min={batch_min}")
    finally:
        set_binary_batch(prev)
        seg.free()
    return ids, dist, st


@pytest.mark.parametrize("route", [3, 4], ids=["popcount", "i8_mfma"])
@pytest.mark.parametrize("nbits", [256, 1024])
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_binary_overflow_nq640(mq, metric, nbits, route):
    """nq 640 (capacity 52224) on the popcount scan (path 3) and, under
    set_binary_batch(1), the i8 MFMA scan (path 4).  The main segments start
    at two probe lengths and grow 4x with a refinement between them
    (search_binary.hip): one of them -- the fifth, [43776, 174848) at a probe
    of 256 rows -- holds more rows strictly under the k-th best of the rows
    before it than a list holds.  So do the 131072 rows after the probe under
    the probe's own k-th best."""
    nq = 640
    ids, dist, st = search_codes(mq, metric, nbits, "worst_first", nq, batch_min=1 if route == 4 else 0)
    assert st["path"] == route, st  # (set by the host before any scan)
    tr = R.trend_codes(NB, nbits, "worst_first")
    d = R.distances_binary(metric, tr.rows, tr.queries)
    P = st["probe_rows"]
    got = R.passing(d, P, BIN_WINDOW, K, strict=True)
    print("passing rows after the probe:", got.min(), "capacity", cand_cap(nq))
    assert got.min() > cand_cap(nq), (P, got.min())
    worst, b, seg_rows = 0, P, max(2 * P, 256)
    while b < NB:  # the plan's segments, restated
        e = min(NB, -(-(b + seg_rows) // 256) * 256)
        worst = max(worst, int(R.passing(d, b, e - b, K, strict=True).min()))
        b, seg_rows = e, 4 * seg_rows
    print("most passing rows of one main segment:", worst)
    assert worst > cand_cap(nq), (P, worst)
    ids_o, dist_o = reference_binary(metric, nbits, "worst_first", nq)
    assert_bitwise(ids, dist, ids_o, dist_o, f"binary overflow {metric} {nbits} path {route}")


@pytest.mark.parametrize("order,nq", [("worst_first", 1), ("worst_first", 8), ("best_first", 640)])
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_binary_parity_on_ordered_rows(mq, metric, order, nq):
    """nq 1 and 8: k_scan_binary_co (capacity 2^20: no overflow); best_first
    at nq 640: the probe's threshold is nearly the final one."""
    ids, dist, _ = search_codes(mq, metric, 256, order, nq)
    ids_o, dist_o = reference_binary(metric, 256, order, nq)
    assert_bitwise(ids, dist, ids_o, dist_o, f"binary {metric} {order} nq={nq}")


# ---- placement: one thread owns the k best probe positions ---------------------------

PN, PK = 32768, 32  # a dense probe of the whole part (n <= 32768, k > 16)
OWNED = np.array([4096 * m + j for m in range(8) for j in range(4)])  # (p >> 2) % 1024 == 0: thread 0's


@lru_cache(maxsize=None)
def placement_part(metric):
    """Gaussian rows, the queries near a centre c, and the 32 rows nearest to
    the queries planted at thread 0's probe positions."""
    rng = np.random.default_rng(zlib.crc32(f"placement_{metric}".encode()))
    rows = rng.standard_normal((PN, D)).astype(np.float32)
    c = rng.standard_normal(D).astype(np.float32)
    near = c[None, :] + 0.01 * rng.standard_normal((len(OWNED), D)).astype(np.float32)
    rows[OWNED] = 4.0 * near if metric == "IP" else near
    q = (c[None, :] + 0.02 * rng.standard_normal((R.NQ_DISTINCT, D))).astype(np.float32)
    return rows, q


def placement_case(mq, metric, nq, k, flt=None, dense=True, **kw):
    rows, q = placement_part(metric)
    qs = R.tile(q, nq) if nq > R.NQ_DISTINCT else q[:nq]
    ids_o, dist_o = O.vector_scan(rows, q[:min(nq, R.NQ_DISTINCT)], k, O.METRICS[metric], GRAN, filter_bits=flt,
                                  fast=True)
    if nq > R.NQ_DISTINCT:
        ids_o, dist_o = R.tile(ids_o, nq), R.tile(dist_o, nq)
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=GRAN)
    try:
        ids, dist = seg.search(qs, k, metric, flt, **kw)
        st = stats(f"placement {metric} nq={nq} k={k} filter={flt is not None}")
    finally:
        seg.free()
    if dense:
        assert st["probe_rows"] == PN, st
    return ids, dist, ids_o, dist_o


@pytest.mark.parametrize("nq", [1, 200])
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_one_thread_holds_the_k_best(mq, metric, nq):
    ids, dist, ids_o, dist_o = placement_case(mq, metric, nq, PK)
    assert set(ids_o[0]) == set(OWNED)  # (the planted rows are the k best)
    assert_bitwise(ids, dist, ids_o, dist_o, f"placement {metric} nq={nq}")


@pytest.mark.parametrize("nq", [1, 200])
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_kept_subset_short_of_k(mq, metric, nq):
    """Masked scan; the filter passes thread 0's positions and 64 random
    rows, k 10 (a short probe: k <= 16): thread 0 keeps 4 of its valid keys,
    most threads none, and the probe holds fewer than k valid rows."""
    rng = np.random.default_rng(zlib.crc32(b"placement_filter"))
    keep = np.zeros(PN, bool)
    keep[OWNED] = True
    keep[rng.choice(PN, 64, replace=False)] = True
    ids, dist, ids_o, dist_o = placement_case(mq, metric, nq, 10, R_pack(keep), dense=False, gather=False)
    assert_bitwise(ids, dist, ids_o, dist_o, f"placement filter {metric} nq={nq}")
