"""The index path (mqvs_index_*) at wide rows: d in {320, 1024, 1216, 1536, 2048,
3072} and the widest accepted, 5056.

The list scan (k_ivf_scan, kernels_ivf_scan.hip) keeps a tile of 16 QB bf16
queries in LDS: 16 QB (2 dpad + 16) bytes of dynamic LDS + 256 QB static.
list_pass (index_search.hip) wants 64-query items when lists average >= 40 probing
queries (E = nq nprobe >= 40 nlist), 32 from 24 and on every dense pass, 16
otherwise, and takes the largest of that size and its smaller siblings that
fits a workgroup's LDS (ivf_fit_qg): with 160 KiB, 64 up to dpad 1216, 32 up
to 2496, 16 up to 5056.  Wider rows are refused by mqvs_index_build.

Its window loop runs ngrp = ceil(dpad / 64 / 4) groups of four 64-column
windows; dpad 320 gives two groups with a one-window tail, 1536 / 2048 / 3072
six, eight and twelve full groups (the suite's other rows: one group).

FLAT at these widths is pinned to the oracle by test_gpu_widths.py; here the
index is pinned to FLAT (exhaustive probing), to itself across the query-group
forms and pair mode, to the re-rank of all candidates (pruning), and its
first-stage values to a float64 reference with a derived rounding bound.
Parts are small (8192 rows of generator mode 2, 16 lists).
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, NLIST = 8192, 16
SEED = 0x5EED0001


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def same_bits(a, b, ctx):
    assert np.array_equal(a[0], b[0]), ctx
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), ctx


EXHAUSTIVE = [(320, "L2", NLIST), (1024, "IP", NLIST), (1536, "L2", NLIST), (1536, "IP", NLIST),
              (1536, "Cosine", NLIST), (2048, "L2", NLIST), (3072, "Cosine", NLIST),
              # more than 64 probes: the coarse step is the dense list pass over the centroid chunks
              (1536, "L2", 128), (3072, "IP", 128)]


@pytest.mark.parametrize("d,metric,nlist", EXHAUSTIVE, ids=[f"d{d}_{m}_nlist{L}" for d, m, L in EXHAUSTIVE])
def test_index_wide_exhaustive_equals_flat(mq, d, metric, nlist):
    """nprobe = nlist, num_reorder 4096: ids, distances, order and padding of
    the FLAT search (as test_index_exhaustive_equals_flat, at wide rows).  nq 5
    scans with 16-query items, nq 24 (E = 24 nlist) with 32-query items (16 at
    dpad 3072, where 32 do not fit).  With 128 lists nprobe is above the
    coarse pick's 64, so the probes come from the dense list pass over the
    centroid chunks (k_plan_dense groups by the item size it is given: 32, or
    16 at dpad 3072); a list it missed would show as rows missing from the
    result."""
    seg = mq.VectorScanSegment.generate(SEED, 2, N, d, metric=metric, granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist})
    try:
        assert idx.info()["rows_indexed"] == N
        for nq in (5, 24):
            q = O.generate(SEED, 2, N, nq, d)
            got = idx.search(q, 50, {"nprobe": nlist, "num_reorder": 4096})
            st = mq.vector_index.last_index_stats()
            assert st["nprobe"] == nlist and st["values"] >= nq * N, st
            same_bits(got, seg.search(q, 50), f"exhaustive d={d} {metric} nq={nq}")
    finally:
        idx.free()
        seg.free()


@pytest.mark.parametrize("d,metric", [(320, "IP"), (1216, "L2"), (1536, "Cosine"), (3072, "L2")])
def test_index_wide_query_group_forms_agree(mq, d, metric):
    """nprobe 4 of 16 lists: the same 40 held-out queries alone (E = 160: 16-
    query items), inside a batch of 100 (E = 400 >= 24 nlist: 32) and of 200
    (E = 800 >= 40 nlist: 64 wanted) return the same ids and distance bits
    (queries are independent; every batch uses the nq >= 20 formula).  d 1216
    is the last dpad at which the 64-query tile fits (156672 B of dynamic LDS,
    above the 64 KiB a kernel gets without opting in).  At
    dpad 1536 the 64-query tile (198656 B) does not fit a workgroup's LDS and
    the pass falls back to 32, at 3072 every pass to 16: no launch is refused."""
    seg = mq.VectorScanSegment.generate(SEED, 2, N, d, metric=metric, granule=1024)
    q = O.generate(SEED, 2, N, 200, d)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": NLIST})
    try:
        out = {}
        for nq in (40, 100, 200):
            out[nq] = idx.search(q[:nq], 30, {"nprobe": 4})
            st = mq.vector_index.last_index_stats()
            assert st["pairs"] == 4 * nq and st["values"] > 0, st
    finally:
        idx.free()
        seg.free()
    assert (out[40][0] >= 0).all()
    for nq in (100, 200):
        same_bits((out[nq][0][:40], out[nq][1][:40]), out[40], f"qg d={d} {metric} batch {nq}")


@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
@pytest.mark.parametrize("plane", ["bf16", "fp8"])
def test_index_64_query_tile_opt_in(mq, plane, metric):
    """The 64-query tile at d 768 needs 64 (2 * 768 + 16) = 99328 B of dynamic
    LDS, above the 65536 B a kernel gets without opting in: launch_ivf_scan
    opts the plane's three scans in before the launch, and a scan it missed
    fails its launch.  2048 rows, 4 lists, nprobe 4, first stage only: queries
    0..2 alone (E = 12: 16-query items) and inside the batch of 40 (E = 160 =
    40 nlist: 64-query items) return the same ids and value bits -- a query's
    first-stage value does not depend on its tile (as
    test_index_wide_pair_mode relies on)."""
    n, d, nlist, k = 2048, 768, 4, 20
    q = O.generate(SEED, 2, n, 40, d)
    seg = mq.VectorScanSegment.generate(SEED, 2, n, d, metric=metric, granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": nlist, "plane": plane})
    try:
        out = {}
        for nq in (3, 40):
            out[nq] = idx.search(q[:nq], k, {"nprobe": 4}, first_stage_only=True)
            st = mq.vector_index.last_index_stats()
            assert st["pairs"] == 4 * nq, st
    finally:
        idx.free()
        seg.free()
    same_bits((out[40][0][:3], out[40][1][:3]), out[3], f"64-query tile {plane} {metric}")


def test_index_wide_pair_mode(mq):
    """Pair mode (16 nq nprobe <= nlist: no plan, one work item per (pair, list
    slice)) at d = 1536 against the grouped plan.
    nlist 64, nq 2, nprobe 2: the two queries alone (pair mode) and inside a
    batch of 40 (grouped).  A batch of 2 re-ranks with the direct formula and
    one of 40 with the BLAS formula, so this pair is compared where no formula
    enters: the first-stage result (ids and the list scan's approximate IP
    values, bit for bit).
    The full search is compared where both runs use one formula, as
    test_index_pair_mode_equals_grouped_plan does: nq 20 (pair mode needs
    16 * 40 <= nlist: 640 lists) against nq 40 with the first 20 shared."""
    d = 1536
    q = O.generate(SEED, 2, N, 40, d)
    seg = mq.VectorScanSegment.generate(SEED, 2, N, d, metric="IP", granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 64})
    try:
        a = idx.search(q[:2], 100, {"nprobe": 2}, first_stage_only=True)
        st = mq.vector_index.last_index_stats()
        b = idx.search(q, 100, {"nprobe": 2}, first_stage_only=True)
    finally:
        idx.free()
        seg.free()
    assert st["pairs"] == 4 and st["values"] > 0, st
    assert (a[0][:, :20] >= 0).all()
    same_bits(a, (b[0][:2], b[1][:2]), "pair mode first stage")

    seg = mq.VectorScanSegment.generate(SEED, 2, N, d, metric="L2", granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 640})
    try:
        a = idx.search(q[:20], 10, {"nprobe": 2})
        st = mq.vector_index.last_index_stats()
        b = idx.search(q, 10, {"nprobe": 2})
    finally:
        idx.free()
        seg.free()
    assert st["pairs"] == 40 and st["values"] > 0, st
    same_bits(a, (b[0][:20], b[1][:20]), "pair mode nq 20 in 40")


@pytest.mark.parametrize("qmode,nq", [(2, 12), (2, 40), (0, 12), (0, 40)])
def test_index_wide_pruned_rerank_equals_full(mq, qmode, nq):
    """Cosine at d = 2048, where the queries are prepared by k_query_prep_lds
    (d > 1536).  The re-rank's bound pruning reads each query's variant spread
    (qdelta) from a workspace buffer that the prep's second phase fills on the
    side stream; the LDS kernel used to return at once in that phase, so the
    pruning read whatever an earlier search had left there.
    qmode 2: held-out mixture queries; qmode 0: small-integer queries, whose
    re-normalisation chains are long, on 32 chunk ordinals, so many variants
    are in use.

    The pruned search returns the bits of re-ranking all num_reorder
    candidates, on both formulas, with a filter and deletes (as
    test_index_pruned_rerank_equals_full at d = 768), and it is a function of
    its own inputs: run after a d = 1536 cosine search of 200 mixture queries
    and again after one of 200 small-integer queries (the register kernel
    leaves those queries' spreads in the same buffer), it re-ranks the same
    number of candidates and returns the same bits.  The spread of finite
    queries is a few 1e-7, small against the bf16 bound, so a stale value
    seldom moves a result; the count is the most sensitive public figure."""
    d, k, R = 2048, 50, 400
    gran = 1024 if qmode == 2 else 256
    seg = mq.VectorScanSegment.generate(SEED, 2, N, d, metric="Cosine", granule=gran)
    q = O.generate(SEED, 2, N, nq, d) if qmode == 2 else O.generate(SEED + 1, 0, 0, nq, d)
    rng = np.random.default_rng(nq)
    flt = np.packbits((rng.random(N) < 0.5).astype(np.uint8), bitorder="little")
    ex = np.packbits((rng.random(N) >= 0.2).astype(np.uint8), bitorder="little")
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": NLIST})
    seg2 = mq.VectorScanSegment.generate(SEED, 2, N, 1536, metric="Cosine", granule=256)
    idx2 = mq.VectorIndex.build(seg2, "MSTG", {"nlist": NLIST})
    try:
        params = {"nprobe": 6, "num_reorder": R}
        full = idx.search(q, k, params, filter_bitmap=flt, row_exists=ex, rerank_all=True)
        st_a = mq.vector_index.last_index_stats()
        runs = []
        for pre_mode in (2, 0):
            idx2.search(O.generate(SEED + 2, pre_mode, 0, 200, 1536), 10, {"nprobe": 4})
            pruned = idx.search(q, k, params, filter_bitmap=flt, row_exists=ex)
            runs.append((pruned, mq.vector_index.last_index_stats()["reranked"]))
    finally:
        idx2.free()
        seg2.free()
        idx.free()
        seg.free()
    assert st_a["reranked"] == nq * R
    for pruned, cnt in runs:
        same_bits(pruned, full, f"pruned qmode={qmode} nq={nq}")
        assert 0 < cnt <= nq * R, cnt
    assert runs[0][1] == runs[1][1], runs[0][1:] + runs[1][1:]
    if qmode == 2:
        assert runs[0][1] < nq * R, runs[0][1]


def _bf16(x):
    """f32_to_bf16_rn (flat_kernels.h): round to nearest even, as float64."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("d", [320, 1536])
def test_index_wide_first_stage_values(mq, d, metric):
    """first_stage_only, exhaustive, nq 24, k 200: every returned (query, row)
    value against float64 arithmetic on the operands the kernel reads.

    Operands: a = bf16(query) (launch_to_bf16 -> k_to_bf16) and b = bf16(row)
    (k_ivf_pack), both f32_to_bf16_rn, zero in the padding columns.  Value
    (k_ivf_scan's epilogue): IP: acc; L2: (qn + pn) - 2 acc, with acc the fp32
    MFMA accumulation of the dpad products a_i b_i and qn, pn the fp32 squared
    norms of the unrounded query and row.  Reference: dot = sum a_i b_i in
    float64 (IP), |q|^2 + |y|^2 - 2 dot in float64 (L2).

    Bound.  A product of two bf16 values has 16 significant bits: exact in
    fp32.  acc is reached by dpad - 1 additions in an order the MFMA chain
    fixes; each commits a relative error eps of a partial sum no larger than
    S = sum |a_i| |b_i|, so |acc - dot| <= (dpad - 1) eps S to first order.
    eps = 2^-24 for round to nearest; the MFMA's internal adder is not
    documented to round to nearest, so a truncating one is allowed for:
    eps = 2^-23, i.e. |acc - dot| <= c dpad 2^-24 S with c = 2.  L2 doubles
    that term (2 acc is exact) and adds: the fp32 norms, each a sum of d
    squares, c d 2^-24 (qn + pn) by the same argument; and the two roundings of
    (qn + pn) - 2 acc, 2^-24 each of magnitudes <= qn + pn + 2 S.
        tol_IP = c dpad 2^-24 S
        tol_L2 = 2 c dpad 2^-24 S + c d 2^-24 (qn + pn) + 2 2^-24 (qn + pn + 2 S)
    The selection is checked with the same bound: a row outside the returned
    200 had a computed value no better than the 200th's, so its reference is
    no better than the 200th's by more than the sum of the two tolerances."""
    nq, k, c, u = 24, 200, 2.0, 2.0 ** -24
    dpad = (d + 63) // 64 * 64
    rows = O.generate(SEED, 2, 0, N, d)
    q = O.generate(SEED, 2, N, nq, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=1024)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": NLIST})
    try:
        ids, val = idx.search(q, k, {"nprobe": NLIST}, first_stage_only=True)
    finally:
        idx.free()
        seg.free()
    a, b = _bf16(q), _bf16(rows)
    dot = a @ b.T
    S = np.abs(a) @ np.abs(b).T
    if metric == "IP":
        ref, tol = dot, c * dpad * u * S
    else:
        nn = (q.astype(np.float64) ** 2).sum(1)[:, None] + (rows.astype(np.float64) ** 2).sum(1)[None, :]
        ref = nn - 2 * dot
        tol = 2 * c * dpad * u * S + c * d * u * nn + 2 * u * (nn + 2 * S)
    assert (ids >= 0).all() and (ids < N).all()
    qi = np.arange(nq)[:, None]
    assert all(len(set(r)) == k for r in ids.tolist())
    err = np.abs(val.astype(np.float64) - ref[qi, ids])
    ratio = (err / tol[qi, ids]).max()
    print(f"first stage d={d} {metric}: max |value - ref| = {err.max():.3e}, largest error / bound = {ratio:.3e}")
    assert ratio <= 1.0, (d, metric, ratio)
    # the returned rows are the best 200: ascending L2, descending IP
    sgn = 1.0 if metric == "L2" else -1.0
    outside = np.ones((nq, N), bool)
    outside[qi, ids] = False
    kth_ref, kth_tol = ref[qi, ids][:, -1:], tol[qi, ids][:, -1:]
    slack = sgn * (ref - kth_ref) + tol + kth_tol   # >= 0 unless an outside row beats the 200th beyond rounding
    assert (slack[outside] >= 0).all(), (d, metric, slack[outside].min())


def test_index_widest_accepted_rows(mq):
    """d = 5056, the widest rows mqvs_index_build accepts: the 16-query tile is
    16 (2 * 5056 + 16) = 162048 B of dynamic LDS + 256 B static, 1536 B under
    the workgroup's 163840.  A 512-row part, exhaustive: the index equals FLAT
    and FLAT equals the oracle, bit for bit."""
    n, d, k = 512, 5056, 20
    rows = O.generate(SEED, 2, 0, n, d)
    q = O.generate(SEED, 2, n, 5, d)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=128)
    idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": 4})
    try:
        got = idx.search(q, k, {"nprobe": 4, "num_reorder": 512})
        flat = seg.search(q, k)
    finally:
        idx.free()
        seg.free()
    same_bits(got, flat, "d 5056 exhaustive")
    same_bits(flat, O.vector_scan(rows, q, k, O.L2, 128, fast=True), "d 5056 FLAT vs oracle")


def test_index_build_refuses_rows_wider_than_the_scan_tile(mq):
    """d = 5100 (dpad 5120): a 16-query tile is 16 (2 * 5120 + 16) + 256 =
    164352 B, above the 163840 B of a workgroup; mqvs_index_build refuses with
    BAD_ARGUMENTS and names the limit (5056 dimensions) before any work."""
    from myscaledb_amd._lib import MqvsError
    rows = O.generate(SEED, 1, 0, 64, 5100)
    seg = mq.VectorScanSegment.from_rows(rows, metric="L2", granule=64)
    try:
        with pytest.raises(MqvsError, match="at most 5056 dimensions") as e:
            mq.VectorIndex.build(seg, "MSTG", {"nlist": 4})
        assert e.value.name == "BAD_ARGUMENTS"
    finally:
        seg.free()
