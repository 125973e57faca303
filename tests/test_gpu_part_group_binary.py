"""Binary part groups (mqvs_part_group_search_binary /
myscaledb_amd.BinaryPartGroup): many small FixedString parts searched in one
fused call return, bit for bit, the per-part searches merged by the
reference's cross-part rule -- checked against the CPU oracle
(O.vector_scan_binary per part, then O.merge_parts per query) and against the
library's own per-part search + merge_shards(part_merge=True)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028235e38)
TIE_SIZES = (1, 255, 256, 257, 700, 3000)  # tile length +-1, a one-row part, parts shorter than k
GRAN = 256


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def rand_codes(rng, n, nbytes, density):
    """(n, nbytes) uint8 codes whose bits are set with probability `density`"""
    return np.packbits(rng.random((n, nbytes * 8)) < density, axis=1)


def bits(mask):
    return np.packbits(np.asarray(mask).astype(np.uint8), bitorder="little")


def oracle_group(parts, queries, k, metric, filters=None, exists=None, offsets=None):
    """(part, ids, dist) [nq, k] of the reference: every part scanned on its
    own, the lists merged per query in part order; also the per-part lists."""
    m = O.METRICS[metric]
    nq = queries.shape[0]
    lists = []
    for p, codes in enumerate(parts):
        ids, dist = O.vector_scan_binary(codes, queries, k, m, GRAN,
                                         filter_bits=None if filters is None else filters[p],
                                         row_exists_bits=None if exists is None else exists[p])
        if offsets is not None:
            ids = np.where(ids >= 0, ids + offsets[p], ids)
        lists.append((ids, dist))
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


def make_group(mq, parts, metric="Hamming", offsets=None):
    segs = [mq.BinaryVectorScanSegment.from_codes(c, metric=metric, granule=GRAN,
                                                  row_offset=0 if offsets is None else offsets[p])
            for p, c in enumerate(parts)]
    return segs, mq.BinaryPartGroup(segs)


def free_all(group, segs):
    group.free()
    for s in segs:
        s.free()


def check_padding(got):
    part, ids, dist = got
    pad = ids < 0
    assert np.all(part[pad] == -1) and np.all(ids[pad] == -1) and np.all(dist[pad] == FLT_MAX)
    assert np.all(part[~pad] >= 0)


# ---------------------------------------------------------------- 1. ties
def cross_part_tie(part, dist, q):
    """equal distances from different parts next to each other in query q"""
    v = part[q] >= 0
    return bool(np.any(v[:-1] & v[1:] & (dist[q, :-1] == dist[q, 1:]) & (part[q, :-1] != part[q, 1:])))


def cut_tie(lists, dist, q, k):
    """more rows reach the k-th distance than the result holds"""
    kth = dist[q, k - 1]
    pool = np.concatenate([l[1][q][l[0][q] >= 0] for l in lists])
    return int(np.sum(pool == kth)) > int(np.sum(dist[q] == kth))


@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
@pytest.mark.parametrize("nq,k", [(1, 10), (3, 25), (9, 300), (40, 300)])
def test_oracle_parity_with_ties(mq, metric, nq, k):
    """4-byte codes: distances take few values, so ties across parts and at
    the k-th cut are everywhere.  nq 1 and 3: the coalesced scan; 9 and 40:
    two and five query passes of the row-per-lane scan."""
    nbytes = 4
    rng = np.random.default_rng(1000 + nbytes + nq + k)
    parts = [rand_codes(rng, n, nbytes, 0.5) for n in TIE_SIZES]
    queries = rand_codes(rng, nq, nbytes, 0.5)
    want, lists = oracle_group(parts, queries, k, metric)
    # the properties these inputs were chosen for, asserted on the oracle's result
    assert all(cross_part_tie(want[0], want[2], q) for q in range(nq)), "inputs lost their cross-part ties"
    cuts = sum(cut_tie(lists, want[2], q, k) for q in range(nq))
    if metric == "Hamming":
        assert cuts == nq, f"inputs lost their ties at the k-th cut ({cuts} of {nq} queries)"
    else:
        assert 2 * cuts > nq, f"inputs lost their ties at the k-th cut ({cuts} of {nq} queries)"
    segs, group = make_group(mq, parts, metric)
    try:
        got = group.search(queries, k)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} nq={nq} k={k}")
    assert st["fused_parts"] == 6 and st["looped_parts"] == 0 and st["redo"] == 0 and st["batch"] == 0
    assert st["fused_rows"] == sum(TIE_SIZES) and st["parts"] == 6 and (st["nq"], st["k"]) == (nq, k)


# ---------------------------------------------------------------- 2. widths
@pytest.mark.parametrize("metric,density", [("Hamming", 0.5), ("Jaccard", 0.3)])
@pytest.mark.parametrize("nq", [2, 12])
@pytest.mark.parametrize("nbytes", [16, 17, 32, 40, 64, 128, 136])
def test_widths(mq, metric, density, nq, nbytes):
    """16-B slices per row: 1, 2 (padded), 2, 3 (no coalesced form), 4, 8, and
    9 (above 1024 bits: rows re-read per query pass)."""
    rng = np.random.default_rng(2000 + nbytes + nq)
    parts = [rand_codes(rng, n, nbytes, density) for n in TIE_SIZES]
    queries = rand_codes(rng, nq, nbytes, density)
    want, _ = oracle_group(parts, queries, 50, metric)
    segs, group = make_group(mq, parts, metric)
    try:
        assert group.info()["d"] == 8 * nbytes
        got = group.search(queries, 50)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} N={nbytes} nq={nq}")
    assert st["fused_parts"] == 6 and st["redo"] == 0


# ---------------------------------------------------------------- 3. bitmaps
@pytest.fixture(scope="module")
def bitmap_parts():
    rng = np.random.default_rng(3000)
    sizes = (300, 100, 40, 277, 500, 64)
    parts = [rand_codes(rng, n, 8, 0.5) for n in sizes]
    filters = [bits(rng.random(sizes[0]) < 0.3), None, None, bits(rng.random(sizes[3]) < 0.5),
               bits(np.zeros(sizes[4], bool)), None]
    exists = [None, bits(rng.random(sizes[1]) >= 0.2), None, bits(rng.random(sizes[3]) >= 0.1), None,
              bits(np.zeros(sizes[5], bool))]
    return parts, filters, exists


@pytest.fixture(scope="module")
def bitmap_reference(bitmap_parts):
    """(nq, metric) -> the oracle's result at k 400 (more than the rows that pass), computed once"""
    parts, filters, exists = bitmap_parts
    rng = np.random.default_rng(3001)
    out = {}
    for nq in (3, 10):
        queries = rand_codes(rng, nq, 8, 0.5)
        for metric in ("Hamming", "Jaccard"):
            out[nq, metric] = (queries, oracle_group(parts, queries, 400, metric, filters, exists)[0])
    return out


@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
@pytest.mark.parametrize("nq", [3, 10])
def test_bitmaps(mq, bitmap_parts, bitmap_reference, metric, nq):
    """Per-part filters and deletes with None entries, a part filtered out, a
    part deleted, and k above every part's rows and above the rows that pass
    in all of them: padding in the lists and in the result."""
    parts, filters, exists = bitmap_parts
    queries, want = bitmap_reference[nq, metric]
    segs, group = make_group(mq, parts, metric)
    try:
        got = group.search(queries, 400, filters=filters, row_exists=exists)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} nq={nq}")
    check_padding(got)
    assert not np.any(np.isin(got[0], (4, 5))), "a part with no selected / no live row returned rows"
    assert np.all(got[1][:, -1] == -1), "inputs lost their padding"
    assert np.all(np.sum(got[0] == 2, axis=1) == 40), "a part shorter than k did not return all its rows"
    assert st["fused_parts"] == 6 and st["looped_parts"] == 0


# ---------------------------------------------------------------- 4. the b < nBit rule
def test_hamming_full_distance_rows(mq):
    """Rows at Hamming distance dim_bits (the complement of the query) are
    never returned by hammings_knn_mc; Jaccard returns them at 1.0."""
    rng = np.random.default_rng(4000)
    queries = rand_codes(rng, 2, 4, 0.5)
    comp = ~queries[0]
    parts = [np.tile(comp, (20, 1)), rand_codes(rng, 300, 4, 0.5)]
    parts[1][123] = comp
    want_h, _ = oracle_group(parts, queries, 320, "Hamming")
    want_j, _ = oracle_group(parts, queries, 320, "Jaccard")
    assert int(np.sum(want_h[1][0] >= 0)) == 299 and int(np.sum(want_j[1][0] >= 0)) == 320
    segs, group = make_group(mq, parts)
    try:
        got_h = group.search(queries, 320, metric="Hamming")
        got_j = group.search(queries, 320, metric="Jaccard")
    finally:
        free_all(group, segs)
    assert_same(got_h, want_h, "Hamming")
    assert_same(got_j, want_j, "Jaccard")
    assert not np.any(got_h[0][0] == 0) and not np.any((got_h[0][0] == 1) & (got_h[1][0] == 123))
    check_padding(got_h)


# ---------------------------------------------------------------- 5. mass ties past the sort capacity
@pytest.fixture(scope="module")
def zero_parts():
    return [np.zeros((5000, 8), np.uint8), np.zeros((5000, 8), np.uint8)]


@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
@pytest.mark.parametrize("k", [600, 4096])
def test_mass_ties(mq, zero_parts, metric, k):
    """10000 equal distances, more than a select sorts in LDS: part, then row."""
    queries = np.array([[0x0F, 0, 0, 0, 0xFF, 1, 0, 0]], np.uint8)
    want, _ = oracle_group(zero_parts, queries, k, metric)
    assert np.all(want[0] == 0) and np.array_equal(want[1][0], np.arange(k)) and np.all(want[2] == want[2][0, 0])
    segs, group = make_group(mq, zero_parts, metric)
    try:
        got = group.search(queries, k)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} k={k}")
    assert st["redo"] == 0 and st["fused_parts"] == 2


# ---------------------------------------------------------------- 6. routes
@pytest.fixture(scope="module")
def route_parts():
    rng = np.random.default_rng(6000)
    parts = [rand_codes(rng, n, 4, 0.5) for n in (300, 700, 400)]
    queries = rand_codes(rng, 3, 4, 0.5)
    return parts, queries


@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_mixed_routes(mq, route_parts, metric):
    """A part above the binary row limit is looped, the rest fused: the same
    result as with every part fused."""
    parts, queries = route_parts
    want, _ = oracle_group(parts, queries, 20, metric)
    segs, group = make_group(mq, parts, metric)
    prev = mq.set_part_group_binary_rows(512)
    try:
        assert group.info()["fusable_parts"] == 2
        mixed = group.search(queries, 20)
        st = group.last_stats()
        assert mq.set_part_group_binary_rows(prev) == 512
        assert group.info()["fusable_parts"] == 3
        fused = group.search(queries, 20)
        st_fused = group.last_stats()
    finally:
        mq.set_part_group_binary_rows(prev)
        free_all(group, segs)
    assert_same(mixed, want, f"{metric} mixed")
    assert_same(fused, want, f"{metric} fused")
    assert (st["fused_parts"], st["looped_parts"], st["fused_rows"]) == (2, 1, 700)
    assert (st_fused["fused_parts"], st_fused["looped_parts"], st_fused["fused_rows"]) == (3, 0, 1400)
    assert st["redo"] == 0 and st["batch"] == 0 and st_fused["redo"] == 0 and st_fused["batch"] == 0


def test_large_k_loops_every_part(mq, route_parts):
    parts, queries = route_parts
    want, _ = oracle_group(parts, queries, 5000, "Hamming")
    segs, group = make_group(mq, parts)
    try:
        got = group.search(queries, 5000)
        st = group.last_stats()
    finally:
        free_all(group, segs)
    assert_same(got, want, "k 5000")
    check_padding(got)
    assert (st["fused_parts"], st["looped_parts"], st["fused_rows"]) == (0, 3, 0)
    assert st["redo"] == 0 and st["batch"] == 0


def test_launch_count_independent_of_parts(mq):
    rng = np.random.default_rng(6100)
    parts = [rand_codes(rng, 300 + 17 * p, 32, 0.5) for p in range(12)]
    queries = rand_codes(rng, 2, 32, 0.5)
    launches = []
    for m in (2, 12):
        want, _ = oracle_group(parts[:m], queries, 10, "Hamming")
        segs, group = make_group(mq, parts[:m])
        try:
            got = group.search(queries, 10)
            st = group.last_stats()
        finally:
            free_all(group, segs)
        assert_same(got, want, f"{m} parts")
        assert st["fused_parts"] == m and st["redo"] == 0 and st["batch"] == 0
        launches.append(st["launches"])
    assert launches[0] == launches[1] and launches[0] > 0


# ---------------------------------------------------------------- 7. slices
def test_scratch_budget_slices(mq):
    """nq 64 under a 1 MiB scratch budget: 4096 columns per slice, so the six
    parts (4469 rows) run as two slices -- one more scan and one more select."""
    from myscaledb_amd.vector_scan import set_scratch_budget
    rng = np.random.default_rng(7000)
    parts = [rand_codes(rng, n, 4, 0.5) for n in TIE_SIZES]
    queries = rand_codes(rng, 64, 4, 0.5)
    want, _ = oracle_group(parts, queries, 100, "Jaccard")
    segs, group = make_group(mq, parts, "Jaccard")
    prev = set_scratch_budget(1 << 20)
    try:
        got = group.search(queries, 100)
        st = group.last_stats()
        set_scratch_budget(prev)
        whole = group.search(queries, 100)
        st_whole = group.last_stats()
    finally:
        set_scratch_budget(prev)
        free_all(group, segs)
    assert_same(got, want, "two slices")
    assert_same(whole, want, "one slice")
    assert st["fused_parts"] == 6 and st_whole["fused_parts"] == 6
    assert st["launches"] == st_whole["launches"] + 2


# ---------------------------------------------------------------- 8. row offsets
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_row_offsets(mq, route_parts, metric):
    parts, queries = route_parts
    offsets = [GRAN * 3, GRAN * 40, GRAN * 5]  # granule multiples, not in part order
    want, _ = oracle_group(parts, queries, 30, metric, offsets=offsets)
    segs, group = make_group(mq, parts, metric, offsets=offsets)
    try:
        got = group.search(queries, 30)
    finally:
        free_all(group, segs)
    assert_same(got, want, metric)
    assert np.all(got[1] >= GRAN * 3)


# ---------------------------------------------------------------- 9. device pointers
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_device_pointers(mq, bitmap_parts, bitmap_reference, metric):
    import torch
    parts, filters, exists = bitmap_parts
    queries, want = bitmap_reference[10, metric]
    segs, group = make_group(mq, parts, metric)
    try:
        dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
        tq = torch.from_numpy(queries).cuda()
        tf, te = [dev(f) for f in filters], [dev(e) for e in exists]
        torch.cuda.synchronize()
        got = group.search(tq, 400, filters=tf, row_exists=te)
        assert all(t.is_cuda for t in got)
        got = tuple(t.cpu().numpy() for t in got)
    finally:
        free_all(group, segs)
    assert_same(got, want, f"{metric} device pointers")


# ---------------------------------------------------------------- 10. agreement with the library
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_agrees_with_per_part_search_and_merge(mq, bitmap_parts, bitmap_reference, metric):
    parts, filters, exists = bitmap_parts
    queries, _ = bitmap_reference[3, metric]
    segs, group = make_group(mq, parts, metric)
    try:
        got = group.search(queries, 400, filters=filters, row_exists=exists)
        per = [s.search(queries, 400, None, filters[p], exists[p]) for p, s in enumerate(segs)]
        loop = mq.merge_shards(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), metric,
                               part_merge=True)
    finally:
        free_all(group, segs)
    assert np.array_equal(got[1], loop[0]) and np.array_equal(got[2].view(np.uint32), loop[1].view(np.uint32))


# ---------------------------------------------------------------- 11. errors and the fault drill
def test_errors(mq):
    from myscaledb_amd import _lib
    lib = _lib.lib
    assert lib.mqvs_abi_version() == 4
    rng = np.random.default_rng(11000)
    codes = rand_codes(rng, 300, 8, 0.5)
    queries = rand_codes(rng, 2, 8, 0.5)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming", granule=GRAN)
    seg_j = mq.BinaryVectorScanSegment.from_codes(codes, metric="Jaccard", granule=GRAN)
    seg_w = mq.BinaryVectorScanSegment.from_codes(rand_codes(rng, 300, 16, 0.5), granule=GRAN)
    seg_f = mq.VectorScanSegment.from_rows(O.generate(680, 1, 0, 300, 64), metric="L2", granule=GRAN)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def create_status(handles):
        arr = (ctypes.c_void_p * len(handles))(*handles)
        h = ctypes.c_void_p()
        rc = lib.mqvs_part_group_create(arr, len(handles), ctypes.byref(h))
        assert (rc == _lib.OK) == bool(h.value)
        if h.value:
            lib.mqvs_part_group_free(h)
        return rc

    def search_status(fn, group, q, metric, nq=2, k=5):
        part, ids, dist = np.full((nq, k), 77, np.int32), np.full((nq, k), 77, np.int64), np.full((nq, k), 77, np.float32)
        rc = fn(group._h, p(q), nq, k, metric, None, None, p(part), p(ids), p(dist), 0, None)
        untouched = bool(np.all(part == 77) and np.all(ids == 77) and np.all(dist == 77))
        return rc, untouched

    try:
        # creation: binary and Float32 mixed (either order), differing dim_bits; the default metric is free
        assert create_status([seg._h, seg_f._h]) == _lib.ERR_LOGICAL
        assert create_status([seg_f._h, seg._h]) == _lib.ERR_LOGICAL
        assert create_status([seg._h, seg_w._h]) == _lib.ERR_LOGICAL
        assert create_status([seg._h, seg_j._h]) == _lib.OK
        g = mq.BinaryPartGroup([seg, seg_j])
        fg = mq.PartGroup([seg_f, seg_f])
        try:
            info = g.info()
            assert (info["nparts"], info["rows"], info["d"], info["fusable_parts"], info["hbm_bytes"]) == \
                (2, 600, 64, 2, 0)
            # each call on the other kind of group names the other call
            fq = O.generate(690, 1, 0, 2, 64)
            assert search_status(lib.mqvs_part_group_search, g, fq, _lib.METRIC_L2) == (_lib.ERR_LOGICAL, True)
            assert b"mqvs_part_group_search_binary" in lib.mqvs_last_error()
            assert search_status(lib.mqvs_part_group_search_binary, fg, queries, _lib.METRIC_HAMMING) == \
                (_lib.ERR_LOGICAL, True)
            assert b"mqvs_part_group_search" in lib.mqvs_last_error()
            # a Float32 metric
            assert search_status(lib.mqvs_part_group_search_binary, g, queries, _lib.METRIC_L2) == \
                (_lib.ERR_NOT_IMPLEMENTED, True)
            assert b"Metric not implemented in brute force search for Binary Vector" in lib.mqvs_last_error()
            # a query of another width
            with pytest.raises(_lib.MqvsError) as e:
                g.search(rand_codes(rng, 2, 16, 0.5), 5)
            assert e.value.status == _lib.ERR_LOGICAL
            # an injected device failure is returned with the outputs untouched; the next call is served
            _lib.check(lib.mqvs_inject_fault(_lib.ERR_DEVICE, 1))
            assert search_status(lib.mqvs_part_group_search_binary, g, queries, _lib.METRIC_HAMMING) == \
                (_lib.ERR_DEVICE, True)
            got = g.search(queries, 5, metric="Jaccard")
            assert np.all(got[1] >= 0)
        finally:
            g.free()
            fg.free()
        # nparts * k above the merge's 2^20
        big = mq.BinaryPartGroup([seg] * 65)
        try:
            with pytest.raises(_lib.MqvsError) as e:
                big.search(queries, 16384)
            assert e.value.status == _lib.ERR_BAD_ARGUMENTS
        finally:
            big.free()
    finally:
        for s in (seg, seg_j, seg_w, seg_f):
            s.free()


def test_binary_row_limit_setter(mq):
    """mqvs_set_part_group_binary_rows: returns the previous value, 0 leaves it,
    capped at 2^24; the default is 131072 (profiles/part_group/binary_limit.jsonl)
    and the float limit is its own."""
    prev = mq.set_part_group_binary_rows(0)
    float_limit = mq.set_part_group_rows(0)
    try:
        assert prev == 131072
        assert mq.set_part_group_binary_rows(1 << 30) == prev
        assert mq.set_part_group_binary_rows(100) == 1 << 24
        assert mq.set_part_group_binary_rows(0) == 100
        assert mq.set_part_group_rows(0) == float_limit
    finally:
        mq.set_part_group_binary_rows(prev)
    assert mq.set_part_group_binary_rows(0) == prev


# ---------------------------------------------------------------- 12. the call's frame: refusals and stats
def test_refusals_in_call_order(mq):
    """Status and mqvs_last_error text of every refusal a search raises before
    it looks at the parts, and which one is reported when two apply: the
    checks run in the order of this list."""
    from myscaledb_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(12000)
    seg = mq.BinaryVectorScanSegment.from_codes(rand_codes(rng, 300, 8, 0.5), granule=GRAN)
    seg_f = mq.VectorScanSegment.from_rows(O.generate(1280, 1, 0, 300, 64), metric="L2", granule=GRAN)
    g, fg, big = mq.BinaryPartGroup([seg] * 3), mq.PartGroup([seg_f]), mq.BinaryPartGroup([seg] * 65)
    queries = rand_codes(rng, 1, 8, 0.5)
    part, ids, dist = np.full(16385, 77, np.int32), np.full(16385, 77, np.int64), np.full(16385, 77, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def refusal(group, nq=1, k=3, metric=_lib.METRIC_HAMMING, out_part=True):
        rc = lib.mqvs_part_group_search_binary(group._h if group else None, p(queries), nq, k, metric, None, None,
                                               p(part) if out_part else None, p(ids), p(dist), 0, None)
        return rc, lib.mqvs_last_error().decode()

    bad = _lib.ERR_BAD_ARGUMENTS
    null_group = (bad, "null part group")
    kind = (_lib.ERR_LOGICAL, "Float32 part group: search it with mqvs_part_group_search")
    negative = (bad, "nq and k must be non-negative")
    null_ptr = (bad, "null query or output pointer")
    k_max = (bad, "k above 16384 not supported")
    no_metric = (_lib.ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector")
    too_many = (bad, "nparts * k above 2^20")
    try:
        assert refusal(None) == null_group
        assert refusal(fg) == kind
        assert refusal(g, nq=-1) == negative and refusal(g, k=-1) == negative
        assert refusal(g, out_part=False) == null_ptr
        assert refusal(g, k=16385) == k_max
        assert refusal(g, metric=_lib.METRIC_L2) == no_metric
        assert refusal(big, k=16384) == too_many
        # two at once
        assert refusal(None, nq=-1, out_part=False) == null_group
        assert refusal(fg, nq=-1) == kind and refusal(fg, out_part=False) == kind
        assert refusal(fg, metric=_lib.METRIC_L2) == kind
        assert refusal(g, nq=-1, metric=_lib.METRIC_L2) == negative
        assert refusal(g, k=16385, out_part=False) == k_max
        assert refusal(g, metric=_lib.METRIC_L2, out_part=False) == null_ptr
        assert refusal(big, k=16385) == k_max
        assert refusal(big, k=16384, out_part=False) == null_ptr
        assert refusal(big, k=16384, metric=_lib.METRIC_L2) == no_metric
        assert np.all(part == 77) and np.all(ids == 77) and np.all(dist == 77)
    finally:
        for x in (g, fg, big, seg, seg_f):
            x.free()


@pytest.mark.parametrize("nq", [1, 20])
def test_stats_of_a_mixed_group(mq, nq):
    """Every field of mqvs_part_group_last_stats: parts of 5 and 300 rows
    fused, the part of 700 rows over a row limit of 512 on the per-part route.
    launches: the status fill, one scan and one select (one slice), the merge.
    A call with nq 0 or k 0 leaves the header."""
    from myscaledb_amd import _lib
    rng = np.random.default_rng(12100)
    parts = [rand_codes(rng, n, 8, 0.5) for n in (5, 300, 700)]
    queries = rand_codes(rng, nq, 8, 0.5)
    want, _ = oracle_group(parts, queries, 3, "Hamming")
    segs, group = make_group(mq, parts)
    prev = mq.set_part_group_binary_rows(512)
    try:
        got = group.search(queries, 3)
        st = group.last_stats()
        empty = []
        for n, k in ((0, 3), (nq, 0)):
            _lib.check(_lib.lib.mqvs_part_group_search_binary(group._h, None, n, k, _lib.METRIC_HAMMING, None, None,
                                                              None, None, None, 0, None))
            empty.append(group.last_stats())
    finally:
        mq.set_part_group_binary_rows(prev)
        free_all(group, segs)
    assert_same(got, want, "mixed group")
    assert st == dict(total_ms=0.0, fused_rows=305, parts=3, fused_parts=2, looped_parts=1, launches=4, redo=0,
                      nq=nq, k=3, batch=0)
    header = dict(total_ms=0.0, fused_rows=0, parts=3, fused_parts=0, looped_parts=0, launches=0, redo=0, batch=0)
    assert empty == [dict(header, nq=0, k=3), dict(header, nq=nq, k=0)]
