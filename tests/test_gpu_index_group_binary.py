"""Binary index groups (mqvs_index_group_search_binary /
myscaledb_amd.BinaryIndexGroup): many BINARYMSTG-indexed parts searched in one
fused call return, bit for bit, the per-part index searches merged by the
reference's cross-part rule.  Every result is held to two references:

R1 (independent): per part the centroids and lists read back from the built
    index, the probes computed on the CPU by (Hamming, list id), numpy brute
    force over the rows of the probed lists by (distance, row) with the bitmaps
    and the b < nBit rule, then O.merge_parts per query;
R2 (the contract): the library's per-part BinaryVectorIndex.search with
    nprobe = min(nprobe, nlist_p), then merge_shards(part_merge=True).

Binary distances are exact, so nothing here has a tolerance.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.40282347e+38)
SIZES = (1, 255, 256, 257, 700, 3000)  # a one-row part, the 256-position slice +-1, parts shorter than k
NLISTS = (1, 2, 4, 4, 2, 8)
GRAN = 256
OFFSETS = tuple(GRAN * o for o in (3, 40, 5, 0, 17, 9))  # granule multiples, not in part order
SEED = 5005  # (5004 leaves two of part 3's lists empty with this construction; the properties are asserted below)


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


# ---- numpy restatement of the build and the search (as tests/test_gpu_binary_index.py) ----

def codes_of(rng, n, nbytes, density=0.5):
    bits = rng.random((n, nbytes * 8)) < density
    return np.packbits(bits, axis=1, bitorder="little")


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


def np_cdist(cent_codes, queries):
    return hamming(bits_of(queries), bits_of(cent_codes))


def np_probes(cent_codes, queries, nprobe):
    d = np_cdist(cent_codes, queries)
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


def bits(mask):
    return np.packbits(np.asarray(mask).astype(np.uint8), bitorder="little")


# ---- the inputs ---------------------------------------------------------------------------

def make_parts(seed, nbytes, density, sizes=SIZES):
    """The parts' codes; part 3 is drawn from only 3 distinct codes (so one of
    its 4 lists stays empty)."""
    rng = np.random.default_rng(seed)
    parts = []
    for p, n in enumerate(sizes):
        if p == 3:
            three = codes_of(rng, 3, nbytes, density)
            parts.append(three[rng.integers(3, size=n)])
        else:
            parts.append(codes_of(rng, n, nbytes, density))
    return parts


def default_nprobe(nlist, rows):
    """mqvs.h: the default alpha 3 probes max(4, nlist / 256, 4096 nlist / rows) lists, at most nlist."""
    return int(min(nlist, max(4, -(-nlist // 256), -(-4096 * nlist // rows))))


def part_nprobes(nprobe, nlists=NLISTS, sizes=SIZES):
    return [default_nprobe(L, n) if nprobe is None else min(nprobe, L) for L, n in zip(nlists, sizes)]


class Group:
    """Segments, indexes and the group over `parts`, with what R1 reads back
    from every built index: its centroids and the rows of its lists."""

    def __init__(self, mq, parts, nlists=NLISTS, offsets=OFFSETS):
        self.mq, self.parts, self.nlists, self.offsets = mq, parts, nlists, offsets
        self.segs = [mq.BinaryVectorScanSegment.from_codes(c, metric="Hamming", granule=GRAN, row_offset=offsets[p])
                     for p, c in enumerate(parts)]
        self.idx = [mq.BinaryVectorIndex.build(s, params=f"nlist={nlists[p]},kmeans_iters=8")
                    for p, s in enumerate(self.segs)]
        self.group = mq.BinaryIndexGroup(self.idx)
        self.cent = [ix.centroids() for ix in self.idx]
        self.assign = []
        for p, ix in enumerate(self.idx):
            off, rows = ix.lists()
            a = np.full(len(parts[p]), -1, np.int64)
            for l in range(nlists[p]):
                r = rows[off[l]:off[l + 1]]
                a[r[r >= 0]] = l
            assert np.all(a >= 0)
            self.assign.append(a)
        self.bits = [bits_of(c) for c in parts]
        self.maps = [None] * len(parts)

    def free(self):
        self.group.free()
        for ix in self.idx:
            ix.free()
        for s in self.segs:
            s.free()

    def r1(self, queries, k, metric, nprobe, filters=None, exists=None):
        """(part, ids, dist) and the per-part lists"""
        nq = len(queries)
        nps = part_nprobes(nprobe, self.nlists, [len(c) for c in self.parts])
        lists = []
        for p, codes in enumerate(self.parts):
            n = len(codes)
            want = np_probes(self.cent[p], queries, nps[p])
            allowed = bitmap_mask(None if filters is None else filters[p], n) & \
                bitmap_mask(None if exists is None else exists[p], n)
            rows_ok = [allowed & np.isin(self.assign[p], list(w)) for w in want]
            ids, dist = np_search(self.bits[p], queries, k, metric, rows_ok)
            ids = np.where(ids >= 0, ids + self.offsets[p], ids)
            if self.maps[p] is not None:
                ids = np.where(ids >= 0, self.maps[p][np.maximum(ids, 0)].astype(np.int64), -1)
            lists.append((ids, dist))
        m = O.METRICS[metric]
        part = np.empty((nq, k), np.int32)
        ids = np.empty((nq, k), np.int64)
        dist = np.empty((nq, k), np.float32)
        for q in range(nq):
            part[q], ids[q], dist[q] = O.merge_parts(np.stack([l[0][q] for l in lists]),
                                                     np.stack([l[1][q] for l in lists]), m)
        return (part, ids, dist), lists

    def r2(self, queries, k, metric, nprobe, filters=None, exists=None):
        """(ids, dist) of the per-part searches merged by the library, and the
        sums of their stats words"""
        from myscaledb_amd.vector_index import last_index_stats
        per, sums = [], dict(values=0, items=0, plane_bytes=0, pairs=0)
        for p, ix in enumerate(self.idx):
            params = f"metric={metric}" + ("" if nprobe is None else f",nprobe={min(nprobe, self.nlists[p])}")
            per.append(ix.search(queries, k, params, None if filters is None else filters[p],
                                 None if exists is None else exists[p]))
            st = last_index_stats()
            assert st["nprobe"] == part_nprobes(nprobe, self.nlists, [len(c) for c in self.parts])[p]
            for key in sums:
                sums[key] += st[key]
        merged = self.mq.merge_shards(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), metric,
                                      part_merge=True)
        return merged, sums

    def search(self, queries, k, metric, nprobe, **kw):
        params = f"metric={metric}" + ("" if nprobe is None else f",nprobe={nprobe}")
        return self.group.search(queries, k, params, **kw)


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


def assert_same_r2(got, r2, ctx):
    assert np.array_equal(got[1], r2[0]), f"{ctx}: ids differ from the per-part searches + merge"
    assert np.array_equal(np.asarray(got[2]).view(np.uint32), np.asarray(r2[1]).view(np.uint32)), \
        f"{ctx}: distance bits differ from the per-part searches + merge"


def check_padding(got):
    part, ids, dist = got
    pad = ids < 0
    assert np.all(part[pad] == -1) and np.all(ids[pad] == -1) and np.all(dist[pad] == FLT_MAX)
    assert np.all(part[~pad] >= 0)


def check_both(G, queries, k, metric, nprobe, ctx, filters=None, exists=None, **kw):
    """the group's result held to R1 and R2; returns (result, R1's per-part lists, R2's stats sums, stats)"""
    want, lists = G.r1(queries, k, metric, nprobe, filters, exists)
    r2, sums = G.r2(queries, k, metric, nprobe, filters, exists)
    got = G.search(queries, k, metric, nprobe, filters=filters, row_exists=exists, **kw)
    st = G.group.last_stats()
    assert_same(got, want, f"{ctx} (R1)")
    assert_same_r2(got, r2, ctx)
    check_padding(got)
    return got, lists, sums, st


@pytest.fixture(scope="module")
def base(mq):
    G = Group(mq, make_parts(SEED, 4, 0.5))
    yield G
    G.free()


# ---------------------------------------------------------------- 0. the inputs' properties (CPU restatement)
def test_input_properties(base):
    """What the base shape was chosen for, asserted on the numpy restatement
    of the build (which the built indexes must equal byte for byte)."""
    built = [np_build(c, L, 8) for c, L in zip(base.parts, NLISTS)]
    for p, (cent, assign, _) in enumerate(built):
        assert np.array_equal(cent, base.cent[p]), f"part {p}: centroids differ from the restatement"
        assert np.array_equal(assign, base.assign[p]), f"part {p}: lists differ from the restatement"
    lens = [np.bincount(a, minlength=L) for (_, a, _), L in zip(built, NLISTS)]
    assert int(np.sum(lens[3] == 0)) == 1, "inputs lost their empty list"
    assert lens[4].max() > 256 and lens[5].max() > 256, "inputs lost their lists of two slices"
    info = [ix.info() for ix in base.idx]
    assert [i["max_list"] for i in info] == [int(l.max()) for l in lens]
    ginfo = base.group.info()
    assert (ginfo["nparts"], ginfo["rows"], ginfo["dim_bits"], ginfo["lists"], ginfo["hbm_bytes"]) == \
        (6, sum(SIZES), 32, sum(NLISTS), 0)


def probe_cut_ties(G, queries, nprobe):
    """parts in which some query's nprobe-th and (nprobe + 1)-th nearest centroids are at one distance"""
    parts = 0
    for p, L in enumerate(G.nlists):
        if nprobe >= L:
            continue
        d = np.sort(np_cdist(G.cent[p], queries), axis=1)
        parts += bool(np.any(d[:, nprobe - 1] == d[:, nprobe]))
    return parts


# ---------------------------------------------------------------- 1. ties and cuts
def cross_part_tie(part, dist, q):
    """equal distances from different parts next to each other in query q"""
    v = part[q] >= 0
    return bool(np.any(v[:-1] & v[1:] & (dist[q, :-1] == dist[q, 1:]) & (part[q, :-1] != part[q, 1:])))


def cut_tie(lists, dist, q, k):
    """more rows reach the k-th distance than the result holds"""
    kth = dist[q, k - 1]
    pool = np.concatenate([l[1][q][l[0][q] >= 0] for l in lists])
    return int(np.sum(pool == kth)) > int(np.sum(dist[q] == kth))


def tie_queries(nq, k):
    return codes_of(np.random.default_rng(5100 + nq + k), nq, 4, 0.5)


def test_probe_cut_ties(base):
    """centroid-distance ties at the nprobe cut, in several parts, for the queries of the cases below"""
    for nq, k in [(3, 25), (9, 300), (40, 300)]:
        for nprobe in (1, 3):
            assert probe_cut_ties(base, tie_queries(nq, k), nprobe) >= 2, "inputs lost their ties at the nprobe cut"


@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
@pytest.mark.parametrize("nprobe", [1, 3, 8, None], ids=["nprobe1", "nprobe3", "nprobe8", "default"])
@pytest.mark.parametrize("nq,k", [(1, 10), (3, 25), (9, 300), (40, 300)])
def test_ties_and_cuts(base, metric, nprobe, nq, k):
    """4-byte codes: distances take few values, so results tie across parts and
    at the k-th cut.  nprobe 8 is cut to nlist in five of the six parts (the
    exhaustive slots); the default resolves per part."""
    queries = tie_queries(nq, k)
    res, lists, sums, st = check_both(base, queries, k, metric, nprobe, f"{metric} nprobe={nprobe} nq={nq} k={k}")
    # the properties these inputs were chosen for, on R1's result (which res equals): in most queries
    # equal distances from different parts meet, and more rows reach the k-th distance than are
    # returned.  (One Jaccard query alone may have neither: 32-bit codes give it many distinct values.)
    ties = sum(cross_part_tie(res[0], res[2], q) for q in range(nq))
    cuts = sum(cut_tie(lists, res[2], q, k) for q in range(nq))
    if metric == "Hamming" or nq > 1:
        assert 2 * ties > nq, f"inputs lost their cross-part ties ({ties} of {nq} queries)"
        assert 2 * cuts > nq, f"inputs lost their ties at the k-th cut ({cuts} of {nq} queries)"
    assert st["fused_parts"] == 6 and st["looped_parts"] == 0 and st["parts"] == 6
    assert (st["nq"], st["k"]) == (nq, k) and st["launches"] > 0
    assert {key: st[key] for key in sums} == sums


# ---------------------------------------------------------------- 2. widths
@pytest.mark.parametrize("metric,density", [("Hamming", 0.5), ("Jaccard", 0.3)])
@pytest.mark.parametrize("nq", [2, 12])
@pytest.mark.parametrize("nbytes", [16, 17, 32, 40, 64, 128, 136])
def test_widths(mq, metric, density, nq, nbytes):
    """16-B slices per code: 1, 2 (padded), 2, 3 (a position per lane), 4, 8, 9 (a position per lane)."""
    G = Group(mq, make_parts(2000 + nbytes, nbytes, density))
    try:
        assert G.group.info()["dim_bits"] == 8 * nbytes
        queries = codes_of(np.random.default_rng(2100 + nbytes + nq), nq, nbytes, density)
        _, _, sums, st = check_both(G, queries, 50, metric, 2, f"{metric} N={nbytes} nq={nq}")
    finally:
        G.free()
    assert st["fused_parts"] == 6 and {key: st[key] for key in sums} == sums


# ---------------------------------------------------------------- 3. bitmaps
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
@pytest.mark.parametrize("nq", [3, 10])
def test_bitmaps(base, metric, nq):
    """Per-part filters and deletes with None entries, a part filtered out, a
    part deleted, and k above the rows that pass: padding in the lists and in
    the result."""
    rng = np.random.default_rng(3000 + nq)
    filters = [None, bits(rng.random(SIZES[1]) < 0.3), None, bits(rng.random(SIZES[3]) < 0.5),
               bits(np.zeros(SIZES[4], bool)), bits(rng.random(SIZES[5]) < 0.05)]
    exists = [None, None, bits(rng.random(SIZES[2]) >= 0.2), bits(rng.random(SIZES[3]) >= 0.1), None, None]
    exists[2] = bits(np.zeros(SIZES[2], bool))
    queries = codes_of(rng, nq, 4, 0.5)
    got, _, _, st = check_both(base, queries, 700, metric, 3, f"{metric} nq={nq}", filters, exists)
    assert not np.any(np.isin(got[0], (2, 4))), "a part with no selected / no live row returned rows"
    assert np.all(got[1][:, -1] == -1), "inputs lost their padding"
    assert st["fused_parts"] == 6 and st["looped_parts"] == 0


# ---------------------------------------------------------------- 4. row-ids map
def test_row_ids_map(mq):
    """A map on two parts, one of them registered after the group was created."""
    G = Group(mq, make_parts(SEED, 4, 0.5))
    try:
        queries = codes_of(np.random.default_rng(4000), 5, 4, 0.5)
        for p in (1, 5):
            span = OFFSETS[p] + SIZES[p]
            G.maps[p] = (np.arange(span, dtype=np.uint64) * 7 + 3) % np.uint64(span) + np.uint64(1000 * p)
        G.idx[1].set_row_ids_map(G.maps[1])
        plain = mq.BinaryIndexGroup(G.idx)   # created after part 1's map, before part 5's
        G.idx[5].set_row_ids_map(G.maps[5])
        try:
            for metric in ("Hamming", "Jaccard"):
                want, _ = G.r1(queries, 40, metric, 3)
                r2, _ = G.r2(queries, 40, metric, 3)
                got = plain.search(queries, 40, f"metric={metric},nprobe=3")
                assert_same(got, want, f"{metric} row-ids map (R1)")
                assert_same_r2(got, r2, f"{metric} row-ids map")
                assert np.any(got[0] == 5) and np.any(got[0] == 1)
        finally:
            plain.free()
    finally:
        G.free()


# ---------------------------------------------------------------- 5. routes
def test_large_k_loops_every_part(base):
    queries = codes_of(np.random.default_rng(5000), 3, 4, 0.5)
    got, _, _, st = check_both(base, queries, 5000, "Hamming", 3, "k 5000")
    assert (st["fused_parts"], st["looped_parts"]) == (0, 6)
    assert (st["values"], st["items"], st["plane_bytes"], st["pairs"]) == (0, 0, 0, 0)


def test_scratch_budget_routes(mq):
    """nq 40 under a 1 MiB scratch budget, every list probed (8 B per record):
    parts 0 - 4 (1469 records per query) are one slice, part 5 (3000) the next,
    and a seventh part of 4000 rows passes the budget on its own (1.28 MB) and
    runs per part.  The same bits as with the default budget, where all seven
    are one fused slice."""
    from myscaledb_amd.vector_scan import set_scratch_budget
    sizes, nlists = SIZES + (4000,), NLISTS + (2,)
    G = Group(mq, make_parts(5200, 4, 0.5, sizes), nlists, OFFSETS + (GRAN * 100,))
    try:
        queries = codes_of(np.random.default_rng(5201), 40, 4, 0.5)
        want, _ = G.r1(queries, 100, "Jaccard", 8)
        r2, _ = G.r2(queries, 100, "Jaccard", 8)
        prev = set_scratch_budget(1 << 20)
        try:
            got = G.search(queries, 100, "Jaccard", 8)
            st = G.group.last_stats()
        finally:
            set_scratch_budget(prev)
        whole = G.search(queries, 100, "Jaccard", 8)
        st_whole = G.group.last_stats()
    finally:
        G.free()
    assert_same(got, want, "1 MiB budget (R1)")
    assert_same_r2(got, r2, "1 MiB budget")
    assert_same(whole, got, "default budget")
    assert (st["fused_parts"], st["looped_parts"]) == (6, 1)
    assert (st_whole["fused_parts"], st_whole["looped_parts"]) == (7, 0)
    # one more slice: one more pick, scan and select (every slot probes all its lists: no distance kernel)
    assert st["launches"] == st_whole["launches"] + 3


def test_launch_count_independent_of_parts(mq, base):
    queries = codes_of(np.random.default_rng(5300), 2, 4, 0.5)
    check = lambda G, n: check_both(G, queries, 10, "Hamming", 3, f"{n} parts")[3]
    st6 = check(base, 6)
    G = Group(mq, base.parts[:3], NLISTS[:3], OFFSETS[:3])
    try:
        st3 = check(G, 3)
    finally:
        G.free()
    assert st3["fused_parts"] == 3 and st6["fused_parts"] == 6
    assert st3["launches"] == st6["launches"] and st3["launches"] > 0


# ---------------------------------------------------------------- 6. device pointers
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_device_pointers(base, metric):
    import torch
    rng = np.random.default_rng(6000)
    filters = [None, bits(rng.random(SIZES[1]) < 0.5), None, None, bits(rng.random(SIZES[4]) < 0.5), None]
    exists = [None, None, None, bits(rng.random(SIZES[3]) >= 0.2), None, bits(rng.random(SIZES[5]) >= 0.2)]
    queries = codes_of(rng, 10, 4, 0.5)
    host = base.search(queries, 60, metric, 3, filters=filters, row_exists=exists)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    tq, tf, te = dev(queries), [dev(f) for f in filters], [dev(e) for e in exists]
    torch.cuda.synchronize()
    got = base.search(tq, 60, metric, 3, filters=tf, row_exists=te)
    assert all(t.is_cuda for t in got)
    assert_same(tuple(t.cpu().numpy() for t in got), host, f"{metric} device pointers")
    want, _ = base.r1(queries, 60, metric, 3, filters, exists)
    assert_same(host, want, f"{metric} host pointers (R1)")


# ---------------------------------------------------------------- 7. the fault drill and errors
def test_errors(mq, base):
    from myscaledb_amd import _lib
    lib = _lib.lib
    assert lib.mqvs_abi_version() == 4
    rng = np.random.default_rng(7000)
    queries = codes_of(rng, 2, 4, 0.5)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def create_status(handles):
        arr = (ctypes.c_void_p * max(len(handles), 1))(*handles)
        h = ctypes.c_void_p()
        rc = lib.mqvs_index_group_create(arr, len(handles), ctypes.byref(h))
        assert (rc == _lib.OK) == bool(h.value)
        if h.value:
            lib.mqvs_index_group_free(h)
        return rc

    def raw_search(params, flags=0, nq=2, k=5):
        part, ids, dist = np.full((nq, k), 77, np.int32), np.full((nq, k), 77, np.int64), np.full((nq, k), 77, np.float32)
        rc = lib.mqvs_index_group_search_binary(base.group._h, p(queries), nq, k, params, None, None, p(part), p(ids),
                                                p(dist), flags, None)
        return rc, (part, ids, dist)

    def search_status(params):
        rc, (part, ids, dist) = raw_search(params)
        untouched = bool(np.all(part == 77) and np.all(ids == 77) and np.all(dist == 77))
        return rc, untouched

    seg_w = mq.BinaryVectorScanSegment.from_codes(codes_of(rng, 300, 16), metric="Hamming", granule=GRAN)
    idx_w = mq.BinaryVectorIndex.build(seg_w, params="nlist=2")
    seg_f = mq.VectorScanSegment.from_rows(O.generate(680, 1, 0, 2000, 64), metric="L2", granule=GRAN)
    idx_f = mq.VectorIndex.build(seg_f, params="nlist=4")
    try:
        # creation
        assert create_status([]) == _lib.ERR_BAD_ARGUMENTS
        assert create_status([base.idx[0]._h, None]) == _lib.ERR_BAD_ARGUMENTS
        assert create_status([base.idx[0]._h, idx_f._h]) == _lib.ERR_NOT_IMPLEMENTED
        assert b"float index groups are not built" in lib.mqvs_last_error()
        assert create_status([base.idx[0]._h, idx_w._h]) == _lib.ERR_LOGICAL
        assert create_status([base.idx[1]._h, base.idx[0]._h]) == _lib.OK
        with pytest.raises(_lib.MqvsError) as e:
            mq.BinaryIndexGroup([])
        assert e.value.status == _lib.ERR_BAD_ARGUMENTS
        # search parameters
        assert search_status(b"metric=L2") == (_lib.ERR_NOT_IMPLEMENTED, True)
        assert search_status(b"beam=3") == (_lib.ERR_BAD_ARGUMENTS, True)
        assert search_status(b"nprobe=0") == (_lib.ERR_BAD_ARGUMENTS, True)
        assert search_status(b"nprobe=5000") == (_lib.ERR_BAD_ARGUMENTS, True)
        assert search_status(b"nprobe=4096,num_reorder=100")[0] == _lib.OK
        # MQVS_F_FIRST_STAGE and MQVS_F_ASYNC change nothing
        rc, plain = raw_search(b"nprobe=3")
        rc_f, flagged = raw_search(b"nprobe=3", _lib.F_FIRST_STAGE | _lib.F_ASYNC)
        assert (rc, rc_f) == (_lib.OK, _lib.OK)
        assert_same(flagged, plain, "FIRST_STAGE | ASYNC")
        # a query of another width
        with pytest.raises(_lib.MqvsError) as e:
            base.group.search(codes_of(rng, 2, 16), 5)
        assert e.value.status == _lib.ERR_LOGICAL
        # an injected device failure is returned with the outputs untouched; the next call is served
        _lib.check(lib.mqvs_inject_fault(_lib.ERR_DEVICE, 1))
        assert search_status(b"nprobe=2") == (_lib.ERR_DEVICE, True)
        got = base.group.search(queries, 5, "nprobe=2,metric=Jaccard")
        assert np.all(got[1] >= 0)
        # nparts * k above the merge's 2^20
        big = mq.BinaryIndexGroup([base.idx[1]] * 65)
        try:
            with pytest.raises(_lib.MqvsError) as e:
                big.search(queries, 16384)
            assert e.value.status == _lib.ERR_BAD_ARGUMENTS
        finally:
            big.free()
    finally:
        idx_w.free()
        idx_f.free()
        seg_w.free()
        seg_f.free()
