"""The fused batch route of part groups (mqvs_set_part_group_batch): calls of
nq >= 20 search the small parts of a group with one grouped fp32 MFMA scan,
one grouped select and the merge, and return, bit for bit, what the per-part
searches merged by the reference's cross-part rule return -- checked against
the CPU oracle (O.vector_scan per part, then O.merge_parts per query) and,
where stated, against the library's own per-part search +
merge_shards(part_merge=True).  The route is off by default; every test that
turns it on restores the setting."""
import contextlib
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle as O

import value_cases as V

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028235e38)
EDGE_SIZES = (1, 127, 128, 129, 700, 3000)  # the 128-row tile +-1, a one-row part, parts shorter than k


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


@contextlib.contextmanager
def batch_route(mq, rows, max_nq=0):
    prev = mq.part_group_batch()
    mq.set_part_group_batch(rows, max_nq)
    try:
        yield
    finally:
        mq.set_part_group_batch(*prev)


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


def assert_same_as_loop(mq, got, segs, queries, k, metric, ctx, filters=None, exists=None):
    """the library's own per-part searches and their part merge: ids and distance bits"""
    per = [s.search(queries, k, None, None if filters is None else filters[p],
                    None if exists is None else exists[p]) for p, s in enumerate(segs)]
    loop = mq.merge_shards(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), metric, part_merge=True)
    assert np.array_equal(got[1], loop[0]), f"{ctx}: ids differ from the per-part searches + merge"
    assert np.array_equal(got[2].view(np.uint32), loop[1].view(np.uint32)), \
        f"{ctx}: distance bits differ from the per-part searches + merge"


def make_group(mq, parts, metric, gran, nonempty=None):
    segs = [mq.VectorScanSegment.from_rows(r, metric=metric, granule=gran,
                                           nonempty=None if nonempty is None else nonempty[p])
            for p, r in enumerate(parts)]
    return segs, mq.PartGroup(segs)


def free_all(group, segs):
    group.free()
    for s in segs:
        s.free()


# ---------------------------------------------------------------- 1. ties and tile edges
@lru_cache(maxsize=None)
def tie_parts():
    return [O.generate(80 + p, 0, 0, n, 8) for p, n in enumerate(EDGE_SIZES)]


def cross_part_tie(part, dist, q):
    """equal distances from different parts next to each other in query q"""
    v = part[q] >= 0
    return bool(np.any(v[:-1] & v[1:] & (dist[q, :-1] == dist[q, 1:]) & (part[q, :-1] != part[q, 1:])))


def cut_tie(lists, dist, q, k):
    """more rows reach the k-th distance than the result holds"""
    kth = dist[q, k - 1]
    pool = np.concatenate([l[1][q][l[0][q] >= 0] for l in lists])
    return int(np.sum(pool == kth)) > int(np.sum(dist[q] == kth))


@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
@pytest.mark.parametrize("nq,k", [(20, 25), (128, 25), (129, 300)])  # (129: a second query block of one query)
def test_oracle_parity_with_ties(mq, metric, nq, k):
    parts = tie_parts()
    queries = O.generate(90, 0, 0, nq, 8)
    want, lists = oracle_group(parts, queries, k, metric, 256)
    # the properties these inputs were chosen for, asserted on the oracle's result
    ties = sum(cross_part_tie(want[0], want[2], q) for q in range(nq))
    if metric != "Cosine" and (nq, k) == (129, 300):
        assert ties == nq, f"inputs lost their cross-part ties ({ties} of {nq} queries)"
        cuts = sum(cut_tie(lists, want[2], q, k) for q in range(nq))
        assert 2 * cuts > nq, f"inputs lost their ties at the k-th cut ({cuts} of {nq} queries)"
    if metric != "Cosine" and (nq, k) == (20, 25):
        assert ties >= 19, f"inputs lost their cross-part ties ({ties} of {nq} queries)"
    if metric == "Cosine" and (nq, k) == (129, 300):
        assert ties > 0, "inputs lost their cross-part ties"
    segs, group = make_group(mq, parts, metric, 256)
    try:
        with batch_route(mq, 1 << 20):
            got = group.search(queries, k)
            st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} nq={nq} k={k}")
    assert st["fused_parts"] == 6 and st["looped_parts"] == 0 and st["batch"] == 1 and st["redo"] == 0
    assert st["fused_rows"] == sum(EDGE_SIZES) and (st["nq"], st["k"]) == (nq, k)


# ---------------------------------------------------------------- 2. widths
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
@pytest.mark.parametrize("d", [37, 100, 1600])  # scalar loads / float4 loads with a partial K stage; the wide query prep
def test_widths(mq, metric, d):
    sizes = (129, 300) if d == 1600 else EDGE_SIZES[:5]
    parts = [O.generate(180 + p, 1, 0, n, d) for p, n in enumerate(sizes)]
    queries = O.generate(190, 1, 0, 20, d)
    want, _ = oracle_group(parts, queries, 50, metric, 256)
    segs, group = make_group(mq, parts, metric, 256)
    try:
        with batch_route(mq, 1 << 20):
            got = group.search(queries, 50)
            st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} d={d}")
    assert st["fused_parts"] == len(sizes) and st["batch"] == 1


# ---------------------------------------------------------------- 3. filters, deletes, empty arrays
@lru_cache(maxsize=None)
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
def test_filters_deletes_empty_arrays(mq, metric):
    parts, nonempty, filters, exists = filtered_parts()
    nq, k = 24, 40
    queries = O.generate(290, 1, 0, nq, 32)
    want, _ = oracle_group(parts, queries, k, metric, 128, filters, exists, nonempty)
    segs, group = make_group(mq, parts, metric, 128, nonempty)
    try:
        with batch_route(mq, 1 << 20):
            got = group.search(queries, k, filters=filters, row_exists=exists)
            st = group.last_stats()
        assert_same_as_loop(mq, got, segs, queries, k, metric, metric, filters, exists)
    finally:
        free_all(group, segs)
    assert_same(got, want, metric)
    assert np.all(got[0] != 3), "a part whose filter selects nothing returned rows"
    if metric == "Cosine":
        # filtered cosine parts take the per-part route; the row_exists-only part is fused
        assert st["fused_parts"] == 1 and st["looped_parts"] == 3 and st["batch"] == 1
    else:
        assert st["fused_parts"] == 4 and st["looped_parts"] == 0 and st["batch"] == 1


# ---------------------------------------------------------------- 4. routing
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_routing(mq, metric):
    from myscaledb_amd import _lib
    parts = [O.generate(480 + p, 1, 0, n, 16) for p, n in enumerate((500, 3000, 800))]
    segs, group = make_group(mq, parts, metric, 256)

    def routes(nq, k=20):
        queries = O.generate(490, 1, 0, nq, 16)
        want, _ = oracle_group(parts, queries, k, metric, 256)
        got = group.search(queries, k)
        st = group.last_stats()
        assert_same(got, want, f"{metric} nq={nq} k={k}")
        return st["fused_parts"], st["looped_parts"], st["batch"]

    try:
        # off by default: a batch call loops every part
        assert mq.part_group_batch() == (0, 0)
        assert routes(20) == (0, 3, 0)
        with batch_route(mq, 1000):
            assert mq.part_group_batch() == (1000, 0)
            assert routes(20) == (2, 1, 1)
            # the small route keeps its own limit (mqvs_set_part_group_rows: all three parts)
            assert routes(3) == (3, 0, 0)
            assert routes(20, 4097) == (0, 3, 0)  # k above the select's sort
            segs[0].set_rows_host(True)
            try:
                assert routes(20) == (1, 2, 1)
            finally:
                segs[0].set_rows_host(False)
        with batch_route(mq, 1000, 64):
            assert mq.part_group_batch() == (1000, 64)
            assert routes(64) == (2, 1, 1)
            assert routes(65) == (0, 3, 0)
            # bad arguments change nothing
            for rows, max_nq in ((-1, 0), ((1 << 24) + 1, 0), (1000, 1), (1000, 19), (1000, -1)):
                assert _lib.lib.mqvs_set_part_group_batch(rows, max_nq) == _lib.ERR_BAD_ARGUMENTS
                assert mq.part_group_batch() == (1000, 64)
            mq.set_part_group_batch(1 << 24, 20)
            assert mq.part_group_batch() == (1 << 24, 20)
        assert mq.part_group_batch() == (0, 0)
        rows = ctypes.c_int64(-1)
        _lib.check(_lib.lib.mqvs_part_group_batch(ctypes.byref(rows), None))
        _lib.check(_lib.lib.mqvs_part_group_batch(None, None))
        assert rows.value == 0
    finally:
        mq.set_part_group_batch(0, 0)
        free_all(group, segs)


# ---------------------------------------------------------------- 5. launch count
def test_launch_count_independent_of_parts(mq):
    parts = [O.generate(580 + p, 1, 0, 300 + 17 * p, 16) for p in range(12)]
    queries = O.generate(590, 1, 0, 32, 16)
    launches = []
    with batch_route(mq, 1 << 20):
        for m in (2, 12):
            segs, group = make_group(mq, parts[:m], "L2", 256)
            try:
                got = group.search(queries, 10)
                st = group.last_stats()
            finally:
                free_all(group, segs)
            want, _ = oracle_group(parts[:m], queries, 10, "L2", 256)
            assert_same(got, want, f"{m} parts")
            assert st["fused_parts"] == m and st["batch"] == 1
            launches.append(st["launches"])
    assert launches[0] == launches[1] and launches[0] > 0


# ---------------------------------------------------------------- 6. slices
def test_scratch_budget_slices(mq):
    """A group whose dense matrix passes the scratch budget runs in slices of
    parts: the same bits as with the whole matrix and as the per-part searches
    and their merge."""
    from myscaledb_amd.vector_scan import set_scratch_budget
    parts = [O.generate(880 + p, 0, 0, n, 8) for p, n in enumerate((6000, 257, 6000, 3000))]
    queries = O.generate(890, 0, 0, 64, 8)
    want, _ = oracle_group(parts, queries, 100, "IP", 256)
    segs, group = make_group(mq, parts, "IP", 256)
    prev = set_scratch_budget(1 << 20)  # 4096 columns of 64 queries
    try:
        with batch_route(mq, 1 << 20):
            got = group.search(queries, 100)
            st = group.last_stats()
            set_scratch_budget(prev)
            whole = group.search(queries, 100)
            st_whole = group.last_stats()
        assert_same_as_loop(mq, got, segs, queries, 100, "IP", "slices")
    finally:
        set_scratch_budget(prev)
        free_all(group, segs)
    assert_same(got, whole, "slices")
    assert_same(got, want, "slices, oracle")
    assert st["fused_parts"] == 4 and st["batch"] == 1 and st_whole["fused_parts"] == 4
    assert st["launches"] > st_whole["launches"]


# ---------------------------------------------------------------- 7. non-finite values
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_non_finite_values(mq, metric):
    """value_cases' specials part (rows with a NaN, +-inf or 3e38 component,
    rows of 3e38, +-1e19, denormals and zeros) between two ordinary parts."""
    c = V.case("specials")
    d = c.rows.shape[1]
    parts = [V.base(700, d), c.rows, V.base(1500, d)]
    queries = np.ascontiguousarray(c.queries[:20])
    want, _ = oracle_group(parts, queries, c.k, metric, c.granule)
    segs, group = make_group(mq, parts, metric, c.granule)
    try:
        with batch_route(mq, 1 << 20):
            got = group.search(queries, c.k)
            st = group.last_stats()
        assert_same_as_loop(mq, got, segs, queries, c.k, metric, metric)
    finally:
        free_all(group, segs)
    assert_same(got, want, metric)
    assert st["fused_parts"] == 3 and st["batch"] == 1


# ---------------------------------------------------------------- 8. device pointers
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_device_pointers(mq, metric):
    import torch
    parts, nonempty, filters, exists = filtered_parts()
    queries = O.generate(290, 1, 0, 24, 32)
    segs, group = make_group(mq, parts, metric, 128, nonempty)
    try:
        with batch_route(mq, 1 << 20):
            host = group.search(queries, 40, filters=filters, row_exists=exists)
            st = group.last_stats()
            dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
            tq = torch.from_numpy(queries).cuda()
            tf, te = [dev(f) for f in filters], [dev(e) for e in exists]
            torch.cuda.synchronize()
            got = group.search(tq, 40, filters=tf, row_exists=te)
            st_dev = group.last_stats()
            got = tuple(t.cpu().numpy() for t in got)
    finally:
        free_all(group, segs)
    assert_same(got, host, f"{metric} device pointers")
    assert st["batch"] == 1 and st_dev["batch"] == 1 and st["fused_parts"] == st_dev["fused_parts"] > 0


# ---------------------------------------------------------------- 9. beyond the default variant table
def test_cosine_long_variant_chain(mq):
    """Small-integer queries whose cosine re-normalisation wanders past the
    default table, on parts of more chunk ordinals than it holds: the batch
    route sizes the table for the part with the most ordinals."""
    parts = [O.generate(780 + p, 0, 0, n, 8) for p, n in enumerate((2600, 300, 4100))]
    queries = O.generate(790, 0, 0, 20, 8)
    want, _ = oracle_group(parts, queries, 30, "Cosine", 64)
    segs, group = make_group(mq, parts, "Cosine", 64)
    try:
        with batch_route(mq, 1 << 20):
            got = group.search(queries, 30)
            st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, "cosine, 65 chunk ordinals")
    assert st["fused_parts"] == 3 and st["batch"] == 1


# ---------------------------------------------------------------- the call's frame: stats
def test_stats_of_a_mixed_group(mq):
    """Every field of mqvs_part_group_last_stats at nq 20 with the batch route
    on up to 512 rows: parts of 5 and 300 rows fused, the part of 700 rows on
    the per-part route.  launches: the status fill and the query prep, one
    scan and one select (one slice), the merge.  With the route off every part
    is looped and only the merge is counted."""
    parts = [O.generate(1180 + p, 1, 0, n, 8) for p, n in enumerate((5, 300, 700))]
    queries = O.generate(1190, 1, 0, 20, 8)
    want, _ = oracle_group(parts, queries, 3, "L2", 256)
    segs, group = make_group(mq, parts, "L2", 256)
    try:
        with batch_route(mq, 512):
            got = group.search(queries, 3)
            st = group.last_stats()
        off = group.search(queries, 3)
        st_off = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, "mixed group")
    assert_same(off, want, "route off")
    assert st == dict(total_ms=0.0, fused_rows=305, parts=3, fused_parts=2, looped_parts=1, launches=5, redo=0,
                      nq=20, k=3, batch=1)
    assert st_off == dict(total_ms=0.0, fused_rows=0, parts=3, fused_parts=0, looped_parts=3, launches=1, redo=0,
                          nq=20, k=3, batch=0)
