"""Width sweep of the FLAT search: every class of the dimension d that selects
a separately compiled kernel, HIP path vs the CPU oracle, bit for bit.

Two seeded generator parts (as run_parity builds them) carry every case:

* the main-scan part, n = 36901: above the 32768 rows at which
  search_internal switches from a dense probe of every row to a probe plus a
  segmented main scan (`FlatSearch::plan_probe` in search.hip,
  `scan_n > 32768`), with a partial last tile and granule (granule 2048 for cosine: 19 chunk ordinals, so several
  query variants are in play).  `main_rows > 0` proves the main scan ran;
* the probe-only part, its first 3001 rows: P = scan_n, so the PROBE
  instantiations alone decide the candidates (`main_rows == 0`).

The stats do not tell which pre-filter kernel ran; these rules select it.

launch_hi_t (kernels_hi.hip:563-594), for the probe and the main scan:
  1. main scan, nq > 128, contiguous rows: the batch kernel k_scan_p4m
     (launch_scan_p4; `batch_kernel == 1` in the stats), any dpad;
  2. nq <= 32 and dpad <= 768 (kHiRegMaxDpad): k_scan_hi_reg<.., NQB, N> with
     N = dpad / 32 (launch_hi_reg, kernels_hi.hip:478-507: one build per
     dpad 64, 128, .. 768), NQB = 1 for nq <= 16 and 2 for 17 .. 32;
  3. else nq <= 64: k_scan_hi<1,2,3>; nq <= 128: k_scan_hi<2,2,3>; more (the
     PROBE scan of a large batch): k_scan_hi<2,4,4> -- runtime loops over
     dpad / 32 stages through a ring of LDS buffers.
  The probe of nq <= 2 queries takes 64-row tiles (`ptile` in
  `FlatSearch::plan_probe` with scan_hi_small_tiles_ok,
  kernels_hi.hip:515-520: the TILE form of the register kernel).
Exact kernels (launch_small_t / launch_mfma_t under batch mode 1 or without
planes, launch_exact_rerank on the default path): float4 rows when
d % 4 == 0, scalar loads otherwise; the one-wave re-rank only when
d % 4 == 0 and nq <= 16.  The re-rank's formula follows faiss: direct below
nq 20, BLAS from 20.
launch_query_prep (kernels_qprep.hip): the register kernel
  k_query_prep<J> with J = 2, 4, 8, 12, 16, 24 for d <= 128, 256, 512, 768,
  1024, 1536; k_query_prep_lds above 1536.

Hence the query counts: nq 2 = 64-row probe tiles + NQB 1; 16 = the NQB 1 edge
and the one-wave re-rank; 19 = NQB 2 with the direct formula; 24 = NQB 2 with
the BLAS formula; 48 / 100 / 140 = k_scan_hi<1,2,3>, <2,2,3> and the batch
kernel (with k_scan_hi<2,4,4> as its dense probe's kernel on short parts).
"""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import assert_bitwise, make_part

pytestmark = pytest.mark.gpu

N_MAIN, N_PROBE, K = 36901, 3001, 50
METRICS = ("L2", "IP", "Cosine")


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def _seed(d, metric):
    return (d * 8 + METRICS.index(metric)) * 0x9E37 + 17


def _inputs(d, metric, mode, n, nq):
    rows, _ = make_part(0x5EED0001 ^ _seed(d, metric), n, d, mode)
    q = O.generate(0x5EED0002 ^ _seed(d, metric), mode, 0, nq, d)
    return rows, q


def _check(mq, seg, rows, q, metric, gran, main, ctx, path=2, batch=None):
    """One search against the oracle + the stats that prove its path."""
    from myscaledb_amd import _lib
    ids_o, dist_o = O.vector_scan(rows, q, K, O.METRICS[metric], gran, fast=True)
    ids_g, dist_g = seg.search(q, K, metric)
    st = _lib.last_search_stats()
    assert st["path"] == path, (ctx, st)
    assert (st["main_rows"] > 0) if main else (st["main_rows"] == 0), (ctx, st)
    if batch is not None:
        assert st["batch_kernel"] == batch, (ctx, st)
    assert_bitwise(ids_g, dist_g, ids_o, dist_o, ctx)


def _gran(metric):
    return 2048 if metric == "Cosine" else 8192


# one d per dpad: full rows, odd d (scalar exact kernels + a padding column),
# d % 4 == 0 short of the pad, and a mostly-padding last 64-column stage
REG = [(dpad, dpad - (0, 1, 4, 60)[(dpad // 64 - 1) % 4]) for dpad in range(64, 769, 64)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dpad,d", REG, ids=[f"dpad{p}_d{d}" for p, d in REG])
def test_register_kernel_widths(mq, dpad, d, metric):
    """k_scan_hi_reg<metric, PROBE / main, NQB 1 / 2, N = dpad / 32> for each
    of its twelve builds (rule 2 above), as the main scan of the 36901-row
    part and as the PROBE scan that decides the 3001-row part; nq 2 also
    takes the 64-row probe tiles.  d % 4 != 0 runs the scalar exact re-rank,
    d % 4 == 0 the float4 one (one wave per query at nq <= 16)."""
    assert (d + 63) // 64 * 64 == dpad
    mode = 1 + (dpad // 64) % 2
    rows, q = _inputs(d, metric, mode, N_MAIN, 24)
    gran = _gran(metric)
    for n, main in ((N_MAIN, True), (N_PROBE, False)):
        seg = mq.VectorScanSegment.from_rows(rows[:n], metric=metric, granule=gran)
        try:
            for nq in (2, 16, 19, 24):
                _check(mq, seg, rows[:n], q[:nq], metric, gran, main, f"reg d={d} {metric} n={n} nq={nq}")
        finally:
            seg.free()


WIDE = [(1024, m) for m in METRICS] + [(1536, m) for m in METRICS] + [(2050, m) for m in METRICS] + [
    (776, "L2"), (1530, "IP"), (3072, "Cosine")]


@pytest.mark.parametrize("d,metric", WIDE, ids=[f"d{d}_{m}" for d, m in WIDE])
def test_wide_rows(mq, d, metric):
    """dpad above 768 leaves the register kernel (rule 2 fails on dpad):
    nq 2 / 19 / 24 / 48 run k_scan_hi<1,2,3>, nq 100 k_scan_hi<2,2,3>, nq 140
    the batch kernel, all with 25 .. 96 stages of 32 columns; cosine above
    1536 prepares its queries in k_query_prep_lds.  d 776 = the first dpad
    past the register builds (832); 1530 and 2050 are not multiples of 4."""
    mode = 1 + (d // 2) % 2
    rows, q = _inputs(d, metric, mode, N_MAIN, 140)
    gran = _gran(metric)
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran)
    try:
        for nq in (2, 19, 24, 48, 100, 140):
            _check(mq, seg, rows, q[:nq], metric, gran, True, f"wide d={d} {metric} nq={nq}",
                   batch=1 if nq == 140 else None)
    finally:
        seg.free()


MID = [(192, 192, "L2"), (448, 447, "IP"), (704, 700, "Cosine")]


@pytest.mark.parametrize("dpad,d,metric", MID, ids=[f"dpad{p}_{m}" for p, _, m in MID])
def test_mid_and_batch_kernels_at_untested_stage_counts(mq, dpad, d, metric):
    """nq above 32 at dpad <= 768 (rule 3, and rule 1 at nq 140): the LDS
    kernels' and the batch kernel's runtime stage loops at 6, 14 and 22
    stages (the suite's other rows give 2, 4, 8 and 24)."""
    rows, q = _inputs(d, metric, 2, N_MAIN, 140)
    gran = _gran(metric)
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran)
    try:
        for nq in (48, 100, 140):
            _check(mq, seg, rows, q[:nq], metric, gran, True, f"mid d={d} {metric} nq={nq}",
                   batch=1 if nq == 140 else None)
    finally:
        seg.free()


QP_EDGES = [(d, 2) for d in (128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 1537)] + [(1025, 0),
                                                                                               (1537, 0)]


@pytest.mark.parametrize("d,mode", QP_EDGES, ids=[f"d{d}_mode{m}" for d, m in QP_EDGES])
def test_query_prep_edges(mq, d, mode):
    """Cosine at both sides of every launch_query_prep split (J = 2 | 4 | 8 |
    12 | 16 | 24 | the LDS kernel) on 3001 rows in 64-row granules: 47 chunk
    ordinals, so the re-normalisation chain's variants are walked.  Mode 0
    (small integers) at d = 1025 and 1537: chains that do not repeat early,
    so J = 24 and the LDS kernel go through their no-repeat and grown-table
    branches (test_cosine_long_normalisation_chains does so at d = 768)."""
    rows, q = _inputs(d, "Cosine", mode, N_PROBE, 24)
    seg = mq.VectorScanSegment.from_rows(rows, metric="Cosine", granule=64)
    try:
        for nq in (3, 24):
            _check(mq, seg, rows, q[:nq], "Cosine", 64, False, f"qprep d={d} mode={mode} nq={nq}")
    finally:
        seg.free()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [1530, 2050])
def test_exact_kernels_wide_rows(mq, d, metric):
    """The exact-kernels-only dispatch at wide rows that are no multiple of 4
    (scalar loads): batch mode 1 on a segment with planes, and a segment built
    without planes (set_prefilter(0)); nq 3 = the VALU kernel with the direct
    formula (path 0), nq 24 = the fp32 MFMA kernel (path 1)."""
    from myscaledb_amd.vector_scan import set_batch_mode, set_prefilter
    mode = 1 + (d // 2) % 2
    rows, q = _inputs(d, metric, mode, N_MAIN, 24)
    gran = _gran(metric)
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran)
    try:
        set_batch_mode(1)
        try:
            for nq in (3, 24):
                _check(mq, seg, rows, q[:nq], metric, gran, True, f"exact batch-mode d={d} {metric} nq={nq}",
                       path=0 if nq < 20 else 1)
        finally:
            set_batch_mode(0)
    finally:
        seg.free()
    set_prefilter(0)
    try:
        seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran)
    finally:
        set_prefilter(2)
    try:
        assert seg.info()["prefilter"] == 0
        for nq in (3, 24):
            _check(mq, seg, rows, q[:nq], metric, gran, True, f"exact no-planes d={d} {metric} nq={nq}",
                   path=0 if nq < 20 else 1)
    finally:
        seg.free()
