"""Part groups (mqvs_part_group_search / myscaledb_amd.PartGroup): many small
parts searched in one fused call return, bit for bit, the per-part searches
merged by the reference's cross-part rule -- checked against the CPU oracle
(O.vector_scan per part, then O.merge_parts per query) and against the
library's own per-part search + merge_shards(part_merge=True)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028235e38)
TIE_SIZES = (1, 255, 256, 257, 700, 3000)  # tile length +-1, a one-row part, parts shorter than k


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def oracle_group(parts, queries, k, metric, gran, filters=None, exists=None, nonempty=None):
    """(part, ids, dist) [nq, k] of the reference: every part scanned on its
    own, the lists merged per query in part order; also the per-part lists."""
    m = O.METRICS[metric]
    nq = queries.shape[0]
    lists = []
    for p, rows in enumerate(parts):
        lists.append(O.vector_scan(rows, queries, k, m, gran,
                                   nonempty=None if nonempty is None else nonempty[p],
                                   filter_bits=None if filters is None else filters[p],
                                   row_exists_bits=None if exists is None else exists[p], fast=True))
    part = np.empty((nq, k), np.int32)
    ids = np.empty((nq, k), np.int64)
    dist = np.empty((nq, k), np.float32)
    for q in range(nq):
        part[q], ids[q], dist[q] = O.merge_parts(np.stack([l[0][q] for l in lists]),
                                                 np.stack([l[1][q] for l in lists]), m)
    return (part, ids, dist), lists


def assert_same(got, want, ctx):
    for name, g, w in zip(("part", "ids", "dist"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name == "dist":
            g, w = g.view(np.uint32), w.view(np.uint32)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            q, j = bad[0]
            raise AssertionError(f"{ctx}: {name} differs in {len(bad)} slots; first at query {q} slot {j}: "
                                 f"got {got[0][q, j]}/{got[1][q, j]}/{got[2][q, j]!r} "
                                 f"want {want[0][q, j]}/{want[1][q, j]}/{want[2][q, j]!r}")


def make_group(mq, parts, metric, gran, nonempty=None):
    segs = [mq.VectorScanSegment.from_rows(r, metric=metric, granule=gran,
                                           nonempty=None if nonempty is None else nonempty[p])
            for p, r in enumerate(parts)]
    return segs, mq.PartGroup(segs)


def free_all(group, segs):
    group.free()
    for s in segs:
        s.free()


# ---------------------------------------------------------------- 1. ties
@pytest.fixture(scope="module")
def tie_parts():
    return [O.generate(80 + p, 0, 0, n, 8) for p, n in enumerate(TIE_SIZES)]


def cross_part_tie(part, dist, q):
    """equal distances from different parts next to each other in query q"""
    v = part[q] >= 0
    return bool(np.any(v[:-1] & v[1:] & (dist[q, :-1] == dist[q, 1:]) & (part[q, :-1] != part[q, 1:])))


def cut_tie(lists, dist, q, k):
    """more rows reach the k-th distance than the result holds"""
    if dist.shape[1] < k:
        return False
    kth = dist[q, k - 1]
    pool = np.concatenate([l[1][q][l[0][q] >= 0] for l in lists])
    return int(np.sum(pool == kth)) > int(np.sum(dist[q] == kth))


@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
@pytest.mark.parametrize("nq,k", [(1, 10), (3, 25), (19, 300)])
def test_oracle_parity_with_ties(mq, tie_parts, metric, nq, k):
    queries = O.generate(90, 0, 0, nq, 8)
    want, lists = oracle_group(tie_parts, queries, k, metric, 256)
    # the property these inputs were chosen for, asserted on the oracle's
    # result: the IP rule (last inserted first) and the cut are exercised
    # (L2 / IP: in every query; cosine: in some queries of the largest case)
    if (nq, k) != (1, 10) and metric != "Cosine":
        assert all(cross_part_tie(want[0], want[2], q) for q in range(nq)), "inputs lost their cross-part ties"
    if (nq, k) == (19, 300) and metric == "Cosine":
        assert any(cross_part_tie(want[0], want[2], q) for q in range(nq)), "inputs lost their cross-part ties"
    if (nq, k) != (1, 10) and metric != "Cosine":
        cuts = sum(cut_tie(lists, want[2], q, k) for q in range(nq))
        assert 2 * cuts > nq, f"inputs lost their ties at the k-th cut ({cuts} of {nq} queries)"
    segs, group = make_group(mq, tie_parts, metric, 256)
    try:
        got = group.search(queries, k)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} nq={nq} k={k}")
    assert st["fused_parts"] == 6 and st["looped_parts"] == 0 and st["redo"] == 0
    assert st["fused_rows"] == sum(TIE_SIZES) and st["parts"] == 6 and (st["nq"], st["k"]) == (nq, k)


# ---------------------------------------------------------------- 2. widths
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
@pytest.mark.parametrize("d", [37, 100])
def test_widths(mq, metric, d):
    parts = [O.generate(180 + p, 1, 0, n, d) for p, n in enumerate(TIE_SIZES)]
    queries = O.generate(190, 1, 0, 2, d)
    want, _ = oracle_group(parts, queries, 50, metric, 256)
    segs, group = make_group(mq, parts, metric, 256)
    try:
        got = group.search(queries, 50)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} d={d}")
    assert st["fused_parts"] == 6


# ---------------------------------------------------------------- 3. filters, deletes, empty arrays
@pytest.fixture(scope="module")
def filtered_parts():
    rng = np.random.default_rng(7)
    sizes = (1000, 6000, 3300, 2500)
    parts = [O.generate(280 + p, 1, 0, n, 32) for p, n in enumerate(sizes)]
    ne = (rng.random(sizes[2]) >= 0.3).astype(np.uint8)
    parts[2][ne == 0] = FLT_MAX
    nonempty = [None, None, ne, None]
    bits = lambda mask: np.packbits(mask.astype(np.uint8), bitorder="little")
    filters = [bits(rng.random(sizes[0]) < 0.3), None, bits(rng.random(sizes[2]) < 0.5),
               bits(np.zeros(sizes[3], bool))]
    exists = [None, bits(rng.random(sizes[1]) >= 0.2), bits(rng.random(sizes[2]) >= 0.1), None]
    return parts, nonempty, filters, exists


@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_filters_deletes_empty_arrays(mq, filtered_parts, metric):
    parts, nonempty, filters, exists = filtered_parts
    nq, k = 4, 40
    queries = O.generate(290, 1, 0, nq, 32)
    want, _ = oracle_group(parts, queries, k, metric, 128, filters, exists, nonempty)
    segs, group = make_group(mq, parts, metric, 128, nonempty)
    try:
        got = group.search(queries, k, filters=filters, row_exists=exists)
        st = group.last_stats()
        per = [s.search(queries, k, None, filters[p], exists[p]) for p, s in enumerate(segs)]
        loop = mq.merge_shards(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), metric,
                               part_merge=True)
    finally:
        free_all(group, segs)
    assert_same(got, want, metric)
    assert np.array_equal(got[1], loop[0]) and np.array_equal(got[2].view(np.uint32), loop[1].view(np.uint32))
    assert np.all(got[0][:, :] != 3), "a part whose filter selects nothing returned rows"
    if metric == "Cosine":
        # filtered cosine parts take the per-part route; the row_exists-only part is fused
        assert st["fused_parts"] == 1 and st["looped_parts"] == 3
    else:
        assert st["fused_parts"] == 4 and st["looped_parts"] == 0


# ---------------------------------------------------------------- 4. all rows equal
@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_all_rows_equal(mq, metric):
    same = np.tile(np.array([[1, 2, -1, 3]], np.float32), (5000, 1))
    parts = [same, O.generate(380, 0, 0, 600, 4)]
    queries = O.generate(390, 0, 0, 2, 4)
    want, _ = oracle_group(parts, queries, 10, metric, 256)
    segs, group = make_group(mq, parts, metric, 256)
    try:
        got = group.search(queries, 10)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, metric)
    # every row of a part is a candidate of its select: no list can overflow
    assert st["redo"] == 0 and st["fused_parts"] == 2


# ---------------------------------------------------------------- 5. mixed routes
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_mixed_routes(mq, metric):
    parts = [O.generate(480 + p, 1, 0, n, 16) for p, n in enumerate((500, 3000, 800))]
    segs, group = make_group(mq, parts, metric, 256)
    prev = mq.set_part_group_rows(1000)
    try:
        assert group.info()["fusable_parts"] == 2
        for nq, fused, looped in ((3, 2, 1), (20, 0, 3)):
            queries = O.generate(490, 1, 0, nq, 16)
            want, _ = oracle_group(parts, queries, 20, metric, 256)
            got = group.search(queries, 20)
            st = group.last_stats()
            assert_same(got, want, f"{metric} nq={nq}")
            assert (st["fused_parts"], st["looped_parts"]) == (fused, looped)
    finally:
        mq.set_part_group_rows(prev)
        free_all(group, segs)
    assert mq.set_part_group_rows(0) == prev


# ---------------------------------------------------------------- 6. launch count
def test_launch_count_independent_of_parts(mq):
    parts = [O.generate(580 + p, 1, 0, 300 + 17 * p, 16) for p in range(12)]
    queries = O.generate(590, 1, 0, 2, 16)
    launches = []
    for m in (2, 12):
        segs, group = make_group(mq, parts[:m], "L2", 256)
        try:
            group.search(queries, 10)
            st = group.last_stats()
        finally:
            free_all(group, segs)
        assert st["fused_parts"] == m
        launches.append(st["launches"])
    assert launches[0] == launches[1] and launches[0] > 0


# ---------------------------------------------------------------- 7. device pointers
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_device_pointers(mq, filtered_parts, metric):
    import torch
    parts, nonempty, filters, exists = filtered_parts
    queries = O.generate(290, 1, 0, 4, 32)
    segs, group = make_group(mq, parts, metric, 128, nonempty)
    try:
        host = group.search(queries, 40, filters=filters, row_exists=exists)
        dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
        tq = torch.from_numpy(queries).cuda()
        tf, te = [dev(f) for f in filters], [dev(e) for e in exists]
        torch.cuda.synchronize()
        got = group.search(tq, 40, filters=tf, row_exists=te)
        got = tuple(t.cpu().numpy() for t in got)
    finally:
        free_all(group, segs)
    assert_same(got, host, f"{metric} device pointers")


# ---------------------------------------------------------------- 8. errors
def test_errors(mq):
    from myscaledb_amd import _lib
    lib = _lib.lib
    rows = O.generate(680, 1, 0, 300, 16)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=256)
    seg_d = mq.VectorScanSegment.from_rows(rows[:, :8].copy(), metric="L2", granule=256)
    seg_c = mq.VectorScanSegment.from_rows(rows, metric="Cosine", granule=256)
    seg_b = mq.BinaryVectorScanSegment.from_codes(np.zeros((64, 8), np.uint8))

    def create_status(handles):
        arr = (ctypes.c_void_p * max(len(handles), 1))(*handles)
        h = ctypes.c_void_p()
        rc = lib.mqvs_part_group_create(arr, len(handles), ctypes.byref(h))
        assert (rc == _lib.OK) == bool(h.value)
        if h.value:
            lib.mqvs_part_group_free(h)
        return rc

    try:
        assert create_status([]) == _lib.ERR_BAD_ARGUMENTS
        assert create_status([seg._h, None]) == _lib.ERR_BAD_ARGUMENTS
        assert create_status([seg._h, seg_b._h]) == _lib.ERR_LOGICAL
        assert create_status([seg._h, seg_d._h]) == _lib.ERR_LOGICAL
        assert create_status([seg._h, seg_c._h]) == _lib.ERR_LOGICAL
        assert create_status([seg._h, seg._h]) == _lib.OK
        ndev = ctypes.c_int()
        _lib.check(lib.mqvs_device_count(ctypes.byref(ndev)))
        if ndev.value >= 2:
            mq.init(1)
            try:
                other = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=256)
            finally:
                mq.init(0)
            try:
                assert create_status([seg._h, other._h]) == _lib.ERR_BAD_ARGUMENTS
            finally:
                other.free()
        queries = O.generate(690, 1, 0, 2, 16)
        # nparts * k above the merge's 2^20
        big = mq.PartGroup([seg] * 65)
        with pytest.raises(_lib.MqvsError) as e:
            big.search(queries, 16384)
        assert e.value.status == _lib.ERR_BAD_ARGUMENTS
        big.free()
        # a cosine group searched with L2
        cg = mq.PartGroup([seg_c, seg_c])
        with pytest.raises(_lib.MqvsError) as e:
            cg.search(queries, 5, metric="L2")
        assert e.value.status == _lib.ERR_LOGICAL
        cg.free()
        # an injected device failure is returned with the outputs untouched
        g = mq.PartGroup([seg, seg])
        part = np.full((2, 5), 77, np.int32)
        ids = np.full((2, 5), 77, np.int64)
        dist = np.full((2, 5), 77, np.float32)
        _lib.check(lib.mqvs_inject_fault(_lib.ERR_DEVICE, 1))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = lib.mqvs_part_group_search(g._h, p(queries), 2, 5, _lib.METRIC_L2, None, None, p(part), p(ids),
                                        p(dist), 0, None)
        assert rc == _lib.ERR_DEVICE
        assert np.all(part == 77) and np.all(ids == 77) and np.all(dist == 77)
        # the next call is served
        got = g.search(queries, 5)
        assert np.all(got[1] >= 0)
        g.free()
    finally:
        for s in (seg, seg_d, seg_c, seg_b):
            s.free()


# ---------------------------------------------------------------- beyond the default variant table, slices
def test_cosine_long_variant_chain(mq):
    """Small-integer queries whose cosine re-normalisation wanders past the
    default table, on parts of more chunk ordinals than it holds: the fused
    route sizes the table for the part with the most ordinals."""
    parts = [O.generate(780 + p, 0, 0, n, 8) for p, n in enumerate((2600, 300, 4100))]
    queries = O.generate(790, 0, 0, 3, 8)
    want, _ = oracle_group(parts, queries, 30, "Cosine", 64)
    segs, group = make_group(mq, parts, "Cosine", 64)
    try:
        got = group.search(queries, 30)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, "cosine, 65 chunk ordinals")
    assert st["fused_parts"] == 3


@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("equal", [False, True])
def test_merge_above_lds_sort(mq, metric, equal):
    """12 parts x k 400 = 4800 records per query, more than the merge sorts in
    LDS: it sorts only the records up to the k-th distance (small-integer rows:
    ties across parts at the cut), or all of them through global memory when
    more than 4096 tie there (every row equal)."""
    sizes = [300 + 20 * p for p in range(12)]
    if equal:
        parts = [np.tile(np.array([[2, 1, 0, 1, 3, 1, 0, 2]], np.float32), (450, 1)) for _ in sizes]
    else:
        parts = [O.generate(980 + p, 0, 0, n, 8) for p, n in enumerate(sizes)]
    queries = np.abs(O.generate(990, 0, 0, 2, 8)) + 1
    want, _ = oracle_group(parts, queries, 400, metric, 256)
    segs, group = make_group(mq, parts, metric, 256)
    try:
        got = group.search(queries, 400)
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} equal={equal}")
    assert np.all(want[1][:, -1] >= 0)


def test_scratch_budget_slices(mq):
    """A group whose dense matrix passes the scratch budget runs in slices of
    parts: the same bits as the per-part searches and their merge."""
    from myscaledb_amd.vector_scan import set_scratch_budget
    parts = [O.generate(880 + p, 0, 0, n, 8) for p, n in enumerate((6000, 257, 6000, 3000))]
    queries = O.generate(890, 0, 0, 19, 8)
    segs, group = make_group(mq, parts, "IP", 256)
    prev = set_scratch_budget(1 << 20)  # 13797 columns of 19 queries
    try:
        got = group.search(queries, 100)
        st = group.last_stats()
        one = set_scratch_budget(prev)
        whole = group.search(queries, 100)
        st_whole = group.last_stats()
        per = [s.search(queries, 100) for s in segs]
        loop = mq.merge_shards(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), "IP", part_merge=True)
    finally:
        set_scratch_budget(prev)
        free_all(group, segs)
    assert one == 1 << 20
    assert_same(got, whole, "slices")
    assert np.array_equal(got[1], loop[0]) and np.array_equal(got[2].view(np.uint32), loop[1].view(np.uint32))
    assert st["fused_parts"] == 4 and st["launches"] > st_whole["launches"]


# ---------------------------------------------------------------- the call's frame: refusals and stats
def test_refusals_in_call_order(mq):
    """Status and mqvs_last_error text of every refusal a search raises before
    it looks at the parts, and which one is reported when two apply: the
    checks run in the order of this list."""
    from myscaledb_amd import _lib
    lib = _lib.lib
    seg = mq.VectorScanSegment.from_rows(O.generate(1080, 1, 0, 300, 8), metric="L2", granule=256)
    seg_b = mq.BinaryVectorScanSegment.from_codes(np.zeros((64, 8), np.uint8))
    g, bg, big = mq.PartGroup([seg] * 3), mq.BinaryPartGroup([seg_b]), mq.PartGroup([seg] * 65)
    queries = O.generate(1090, 1, 0, 1, 8)
    part, ids, dist = np.full(16385, 77, np.int32), np.full(16385, 77, np.int64), np.full(16385, 77, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def refusal(group, nq=1, k=3, metric=_lib.METRIC_L2, out_part=True):
        rc = lib.mqvs_part_group_search(group._h if group else None, p(queries), nq, k, metric, None, None,
                                        p(part) if out_part else None, p(ids), p(dist), 0, None)
        return rc, lib.mqvs_last_error().decode()

    bad = _lib.ERR_BAD_ARGUMENTS
    null_group = (bad, "null part group")
    kind = (_lib.ERR_LOGICAL, "binary (FixedString) part group: search it with mqvs_part_group_search_binary")
    negative = (bad, "nq and k must be non-negative")
    null_ptr = (bad, "null query or output pointer")
    k_max = (bad, "k above 16384 not supported")
    no_metric = (_lib.ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector")
    too_many = (bad, "nparts * k above 2^20")
    try:
        assert refusal(None) == null_group
        assert refusal(bg) == kind
        assert refusal(g, nq=-1) == negative and refusal(g, k=-1) == negative
        assert refusal(g, out_part=False) == null_ptr
        assert refusal(g, k=16385) == k_max
        assert refusal(g, metric=_lib.METRIC_HAMMING) == no_metric
        assert refusal(big, k=16384) == too_many
        # two at once
        assert refusal(None, nq=-1, out_part=False) == null_group
        assert refusal(bg, nq=-1) == kind and refusal(bg, out_part=False) == kind
        assert refusal(bg, metric=_lib.METRIC_HAMMING) == kind
        assert refusal(g, nq=-1, metric=_lib.METRIC_HAMMING) == negative
        assert refusal(g, k=16385, out_part=False) == k_max
        assert refusal(g, metric=_lib.METRIC_HAMMING, out_part=False) == null_ptr
        assert refusal(big, k=16385) == k_max
        assert refusal(big, k=16384, out_part=False) == null_ptr
        assert refusal(big, k=16384, metric=_lib.METRIC_HAMMING) == no_metric
        assert np.all(part == 77) and np.all(ids == 77) and np.all(dist == 77)
    finally:
        for x in (g, bg, big, seg, seg_b):
            x.free()


def test_stats_of_a_mixed_group(mq):
    """Every field of mqvs_part_group_last_stats at nq 1: parts of 5 and 300
    rows fused, the part of 700 rows over a row limit of 512 on the per-part
    route.  launches: the status fill and the query prep, one scan and one
    select (one slice), the merge.  A call with nq 0 or k 0 leaves the header."""
    from myscaledb_amd import _lib
    parts = [O.generate(1180 + p, 1, 0, n, 8) for p, n in enumerate((5, 300, 700))]
    queries = O.generate(1190, 1, 0, 1, 8)
    want, _ = oracle_group(parts, queries, 3, "L2", 256)
    segs, group = make_group(mq, parts, "L2", 256)
    prev = mq.set_part_group_rows(512)
    try:
        got = group.search(queries, 3)
        st = group.last_stats()
        empty = []
        for nq, k in ((0, 3), (1, 0)):
            _lib.check(_lib.lib.mqvs_part_group_search(group._h, None, nq, k, _lib.METRIC_L2, None, None, None, None,
                                                       None, 0, None))
            empty.append(group.last_stats())
    finally:
        mq.set_part_group_rows(prev)
        free_all(group, segs)
    assert_same(got, want, "mixed group")
    assert st == dict(total_ms=0.0, fused_rows=305, parts=3, fused_parts=2, looped_parts=1, launches=5, redo=0,
                      nq=1, k=3, batch=0)
    header = dict(total_ms=0.0, fused_rows=0, parts=3, fused_parts=0, looped_parts=0, launches=0, redo=0, batch=0)
    assert empty == [dict(header, nq=0, k=3), dict(header, nq=1, k=0)]
