"""The seams of the batch pre-filter scan (kernels_p4.hip, k_scan_p4m): the
hand-over between the two MFMA phases of a stage, between the work items of a
workgroup, and the start and end of the stage ring.

The ring's counted wait is one immediate for the whole launch, dummy stages
included, and its bookkeeping sits in MFMA gaps of phase 0.  These cases are
the smallest shapes at which that can go wrong: items of two, three and four
stages (the ring, three stages deep, is then deeper than the item, and the
unrolled stage pair runs zero times or once), 24-stage items, launches whose
workgroups get one item or none (every wait after the prologue is then on a
dummy stage), ragged last tiles, chunks whose tile count does not divide the
workgroups' tile stride, cosine batches on ordinal planes and on the
per-lane variant fallback, and query blocks with padding queries.

Every case asserts that the batch kernel ran (`batch_kernel` of the search
stats) and compares ids and distances bit for bit with the exact fp32 scan
of the same part (set_batch_mode(1)) and with the CPU oracle.

A part of at most 32768 rows never reaches the main scan (its dense probe
covers every row), so the launches of one and of two work items are built as
the last row segment of a part: 65536 + P rows go to the first segment
(search.hip kMinSegRows, P the probe length) and the 256 or 512 rows after
them to a launch of their own.
"""
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


@pytest.fixture(scope="module")
def cus(mq):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=4)
def _gen(seed, mode, n, d):
    return O.generate(seed, mode, 0, n, d)


def _check(mq, rows, q, k, metric, gran, ctx, want=None):
    """GPU search == exact fp32 scan == oracle, bit for bit; returns the stats
    of the pre-filter search.  want: stats fields the shape relies on."""
    from myscaledb_amd import _lib
    from myscaledb_amd.vector_scan import set_batch_mode
    seg = mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran)
    try:
        ids_g, dist_g = seg.search(q, k, metric)
        st = _lib.last_search_stats()
        set_batch_mode(1)
        try:
            ids_e, dist_e = seg.search(q, k, metric)
        finally:
            set_batch_mode(0)
    finally:
        seg.free()
    brief = {f: st[f] for f in ("batch_kernel", "path", "rescans", "segments", "probe_rows", "main_rows")}
    assert st["batch_kernel"] == 1 and st["main_rows"] > 0, brief
    for f, v in (want or {}).items():
        assert st[f] == v, (f, v, brief)
    assert_bitwise(ids_g, dist_g, ids_e, dist_e, ctx + " vs exact scan")
    ids_o, dist_o = O.vector_scan(rows, q, k, O.METRICS[metric], gran, fast=True)
    assert_bitwise(ids_g, dist_g, ids_o, dist_o, ctx + " vs oracle")
    return st


# ---- stage counts: d / 32 stages per item, 256 x CUs rows (one tile per CU)
@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
@pytest.mark.parametrize("d", [64, 96, 128])
def test_short_items(mq, cus, d, metric):
    n, nq = 256 * cus, 256
    rows = _gen(0x5EA70000 + d, 1, n, d)
    q = _gen(0x5EA71000 + d, 1, nq, d)
    _check(mq, rows, q, 10, metric, 8192, f"{d // 32} stages {metric}")


def test_items_of_24_stages(mq, cus):
    n, nq, d = 256 * cus, 256, 768
    rows = _gen(0x5EA70768, 2, n, d)
    q = _gen(0x5EA71768, 2, nq, d)
    _check(mq, rows, q, 10, "Cosine", 8192, "24 stages Cosine")


# ---- ring drain: a launch of one work item and of two (see the module text)
@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("tail", [256, 512])
def test_launch_of_one_and_two_items(mq, tail, metric):
    d, nq, k, probe = 64, 256, 10, 256
    n = 65536 + probe + tail
    rows = _gen(0x5EA72000, 1, 65536 + probe + 512, d)[:n]
    q = _gen(0x5EA73000, 1, nq, d)
    _check(mq, rows, q, k, metric, 8192, f"tail launch of {tail} rows {metric}",
           want={"probe_rows": probe, "segments": 2})


@pytest.mark.parametrize("metric", ["L2", "Cosine"])
@pytest.mark.parametrize("n", [256 * 160 + 1, 256 * 160 + 255])
def test_ragged_last_tile(mq, n, metric):
    d, nq = 64, 256
    rows = _gen(0x5EA74000, 1, 256 * 161, d)[:n]
    q = _gen(0x5EA75000, 1, nq, d)
    _check(mq, rows, q, 10, metric, 8192, f"n {n} {metric}")


# ---- item arithmetic
def test_cosine_partial_last_chunk(mq):
    """Five granules of 8192 rows and 300 rows more: 32 tiles per chunk, the
    last chunk a whole tile and one of 44 rows."""
    d, nq, gran = 64, 256, 8192
    rows = _gen(0x5EA76000, 2, 5 * gran + 300, d)
    q = _gen(0x5EA77000, 2, nq, d)
    _check(mq, rows, q, 10, "Cosine", gran, "5 granules + 300")


def test_cosine_three_tiles_per_chunk(mq):
    """Granule 768: three tiles per chunk, which does not divide the tile
    stride of a workgroup (a multiple of 8)."""
    d, nq, gran = 64, 256, 768
    rows = _gen(0x5EA78000, 1, 60 * gran + 100, d)
    q = _gen(0x5EA79000, 1, nq, d)
    _check(mq, rows, q, 10, "Cosine", gran, "granule 768")


def _ordinal_planes(q, chunks):
    """Planes the batch's re-normalisation chains need over `chunks` chunk
    ordinals (variant o of a query = normalize applied o + 1 times): max mu +
    lcm of the cycle lengths, or None when a chain does not repeat in time."""
    seen = [dict() for _ in range(len(q))]
    mu, lam = [None] * len(q), [None] * len(q)
    v = np.array(q, np.float32)
    for o in range(chunks):
        v = O.normalize(v)
        for j in range(len(q)):
            if mu[j] is not None:
                continue
            key = v[j].tobytes()
            if key in seen[j]:
                mu[j], lam[j] = seen[j][key], o - seen[j][key]
            else:
                seen[j][key] = o
    if any(m is None for m in mu):
        return None
    return max(mu) + functools.reduce(math.lcm, lam, 1)


def test_cosine_several_ordinal_planes(mq):
    """A query whose chain first repeats at step 16 (generator mode 2, seed
    12, d 256, query 259) with 255 ordinary ones: the chunks' queries come
    from at least three distinct ordinal planes."""
    g = _gen(12, 2, 300, 256)
    q = np.concatenate([g[259:260], g[:255]])
    planes = _ordinal_planes(q, 40)
    assert planes is not None and 3 <= planes <= 32, planes
    rows = _gen(77, 2, 40960, 256)
    _check(mq, rows, q, 10, "Cosine", 1024, "ordinal planes")


def test_cosine_per_lane_variants(mq):
    """Small-integer queries at d 768 whose chains do not repeat within the 32
    planes (the long-chain construction of test_gpu_boundary.py): each lane
    picks its query's variant.  80 chunks of 64 rows, one 64-row tile each."""
    n, d, nq, gran = 80 * 64, 768, 256, 64
    q = _gen(0x5EED0002, 0, nq, d)
    planes = _ordinal_planes(q, n // gran)
    assert planes is None or planes > 32, planes
    rows = _gen(0x5EED0001, 0, n, d)
    _check(mq, rows, q, 10, "Cosine", gran, "per-lane variants")


# ---- padding queries (nq not a multiple of 256: thresholds of +inf)
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
@pytest.mark.parametrize("nq", [129, 257, 1000])
def test_padding_queries(mq, nq, metric):
    # (the 256-row probe of this part gives two group maxima per query: k = 2
    # at nq 1000, whose candidate lists are too short for the appends of a
    # threshold looser than that)
    d, k = 64, 10 if nq < 1000 else 2
    rows = _gen(0x5EA7A000, 1, 40960, d)
    q = _gen(0x5EA7B000, 1, 1000, d)[:nq]
    _check(mq, rows, q, k, metric, 8192, f"nq {nq} {metric}")
