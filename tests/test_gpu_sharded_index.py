"""mqvs_index_search_ex and mqvs_sharded_index_search: one part's index over
the ranks of a communicator, on the GPU box's one GPU (loopback ranks, one
thread each, as tests/test_gpu_sharded.py; a 1-rank RCCL communicator).

* mqvs_index_search_ex: the index of a row-range shard searched with the
  exact cosine chunk-ordinal base equals the FLAT search of that shard with
  the same base bit for bit (every shard row a candidate), also when a
  PREWHERE filter empties a chunk BEFORE the shard.
* Every rank searches its own index exhaustively (nprobe = nlist, num_reorder
  = the shard's rows): the merged result equals the ORACLE's scan of the whole
  part bit for bit (C2), on the validated path and on the one-sync fast path.
* Partial probes: the merged result equals mqvs_merge_shards over the ranks'
  own mqvs_index_search_ex results, each with its exact base (C1), for the
  fp8 plane, the first stage and a row-ids map too.
* FLAT and index calls alternate on one communicator.
* Ranks that disagree (params, flags), a rank whose search fails and a binary
  index fail on EVERY rank; the next agreeing call succeeds.

Shards are 4096 rows; every test fails without the two entry points.
"""
import socket
import threading
import zlib

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028235e38)
EXHAUSTIVE = "nprobe=8,num_reorder=4096"


@pytest.fixture(scope="module")
def mq():
    import myscaledb_amd as m
    m.init(0)
    return m


def _run_ranks(nranks, fn):
    """fn(rank) on one thread per rank -> (results, errors), all threads joined."""
    out, errs = [None] * nranks, [None] * nranks

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    th = [threading.Thread(target=body, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
        assert not t.is_alive(), "a rank did not finish (exchange deadlock)"
    return out, errs


def _raise_first(errs):
    for e in errs:
        if e is not None:
            raise e


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[1]).view(np.uint32),
                                                          np.asarray(b[1]).view(np.uint32))


def _chunk_filter(rng, n, gran, filt):
    """As tests/test_gpu_sharded.py: chunk 0 and a middle chunk filtered out whole."""
    keep = rng.random(n) < filt
    keep[0:gran] = False
    mid = (n // gran // 2) * gran
    keep[mid:mid + gran] = False
    return keep


class Part:
    """A part, its bitmaps and its row-range shards with one index per shard."""

    def __init__(self, mq, name, world, n, d, nq, metric, mode, gran, filt=None, lwd=None, empty=0.0,
                 chunk_filter=True, build="nlist=8", salt=0):
        from myscaledb_amd.sharded import chunk_ordinal_base, shard_rows, slice_bitmap
        self.world, self.n, self.d, self.metric, self.gran = world, n, d, metric, gran
        seed = zlib.crc32(name.encode()) + salt
        self.rows = O.generate(0x5EED0001 ^ seed, mode, 0, n, d)
        self.q = O.generate(0x5EED0002 ^ seed, mode, 0, nq, d)
        rng = np.random.default_rng(seed)
        self.ne = None
        if empty:
            self.ne = (rng.random(n) >= empty).astype(np.uint8)
            self.ne[gran:2 * gran] = 0  # an all-empty chunk
            self.rows[self.ne == 0] = FLT_MAX
        self.flt = None
        if filt is not None:
            self.flt = mq.pack_bitmap(_chunk_filter(rng, n, gran, filt) if chunk_filter else rng.random(n) < filt)
        self.rex = mq.pack_bitmap(rng.random(n) >= lwd) if lwd is not None else None
        self.shards = []
        for r in range(world):
            r0, r1 = shard_rows(n, gran, r, world)
            seg = mq.VectorScanSegment.from_rows(self.rows[r0:r1], metric=metric, granule=gran,
                                                 nonempty=None if self.ne is None else self.ne[r0:r1], row_offset=r0)
            self.shards.append({
                "r0": r0, "r1": r1, "seg": seg, "idx": mq.VectorIndex.build(seg, params=build),
                "flt": slice_bitmap(self.flt, n, r0, r1), "rex": slice_bitmap(self.rex, n, r0, r1),
                "base": chunk_ordinal_base(r0, gran, n, self.ne, self.flt, self.rex)})

    def oracle(self, k):
        return O.vector_scan(self.rows, self.q, k, O.METRICS[self.metric], self.gran, nonempty=self.ne,
                             filter_bits=self.flt, row_exists_bits=self.rex, fast=True)

    def free(self):
        for s in self.shards:
            s["idx"].free()
            s["seg"].free()


# ---- 1. mqvs_index_search_ex, no communicator ------------------------------------------------

@pytest.mark.parametrize("filtered", [True, False], ids=["chunk0_filtered", "no_filter"])
def test_index_search_ex_equals_flat_shard_search(mq, filtered):
    from myscaledb_amd import _lib
    from myscaledb_amd.sharded import chunk_ordinal_base, slice_bitmap
    n, d, gran, r0, nq, k = 8192, 32, 1024, 4096, 7, 30
    rows = O.generate(0x1DE0001, 1, 0, n, d)
    q = O.generate(0x1DE0002, 1, 0, nq, d)
    flt = None
    if filtered:
        keep = np.random.default_rng(11).random(n) < 0.7
        keep[0:gran] = False  # chunk 0 of the part is never searched
        flt = mq.pack_bitmap(keep)
    base = chunk_ordinal_base(r0, gran, n, None, flt, None)
    assert base == (3 if filtered else 4)
    sflt = slice_bitmap(flt, n, r0, n)
    seg = mq.VectorScanSegment.from_rows(rows[r0:], metric="Cosine", granule=gran, row_offset=r0)
    idx = mq.VectorIndex.build(seg, params="nlist=8")
    try:
        flat = seg.search(q, k, filter_bitmap=sflt, ord_base=base)
        got = idx.search(q, k, params=EXHAUSTIVE, filter_bitmap=sflt, chunk_ord_base=base)
        assert _same(got, flat)
        import torch
        tg = idx.search(torch.from_numpy(q).cuda(), k, params=EXHAUSTIVE,
                        filter_bitmap=None if sflt is None else torch.from_numpy(sflt).cuda(), chunk_ord_base=base)
        assert _same((tg[0].cpu().numpy(), tg[1].cpu().numpy()), flat)
        # base -1 is mqvs_index_search
        ids = np.empty((nq, k), np.int64)
        dist = np.empty((nq, k), np.float32)
        from myscaledb_amd.vector_scan import _ptr
        _lib.check(_lib.lib.mqvs_index_search(idx._h, _ptr(q), nq, k, EXHAUSTIVE.encode(), _ptr(sflt), None, _ptr(ids),
                                              _ptr(dist), 0, None))
        assert _same(idx.search(q, k, params=EXHAUSTIVE, filter_bitmap=sflt, chunk_ord_base=-1), (ids, dist))
        assert _same(idx.search(q, k, params=EXHAUSTIVE, filter_bitmap=sflt), (ids, dist))
        with pytest.raises(_lib.MqvsError) as ei:
            idx.search(q, k, params=EXHAUSTIVE, chunk_ord_base=2 ** 31)
        assert ei.value.status == _lib.ERR_BAD_ARGUMENTS
    finally:
        idx.free()
        seg.free()


# ---- 2. exhaustive per-rank searches == the oracle over the whole part (C2) ---------------------

LOOP = [
    # name,           world, n,     d,  nq, k,    metric,   mode, gran, filt, chunk_filter, lwd,  empty
    ("cos_w2_filter", 2,     8192,  32, 7,  30,   "Cosine", 1,    1024, 0.7,  True,         0.1,  0.0),
    ("cos_w4_empty",  4,     16384, 24, 5,  40,   "Cosine", 1,    1024, None, True,         0.1,  0.2),
    ("cos_w8_batch",  8,     32768, 16, 22, 25,   "Cosine", 2,    512,  None, True,         None, 0.0),
    ("l2_w4_filter",  4,     16384, 32, 30, 100,  "L2",     1,    2048, 0.5,  False,        0.2,  0.0),
    ("ip_w8_ties",    8,     32768, 8,  3,  50,   "IP",     0,    1024, None, True,         0.1,  0.0),
    ("l2_w2_bigk",    2,     8192,  16, 4,  3000, "L2",     1,    4096, None, True,         None, 0.0),
]
# cosine cases whose guessed bases are wrong (chunk-emptying filter, all-empty chunk)
WRONG_GUESS = {"cos_w2_filter", "cos_w4_empty"}
# per-case change of the data seed, so that the case has power (see the test):
# most fp32 re-normalisation chains reach a fixed point within three steps,
# and a wrong base of 4 instead of 3 then picks an equal query variant; with
# these seeds one query's chain keeps changing up to ordinal 6 (cos_w2_filter)
# and 9 (cos_w4_empty)
SALT = {"cos_w2_filter": 1, "cos_w4_empty": 9}


@pytest.mark.parametrize("cfg", LOOP, ids=[c[0] for c in LOOP])
def test_loopback_exhaustive_index_equals_oracle(mq, cfg):
    from myscaledb_amd import _lib
    from myscaledb_amd.sharded import LoopbackComm
    from myscaledb_amd.vector_scan import merge_shards
    name, world, n, d, nq, k, metric, mode, gran, filt, cfilt, lwd, empty = cfg
    part = Part(mq, name, world, n, d, nq, metric, mode, gran, filt, lwd, empty, cfilt, salt=SALT.get(name, 0))
    io, do = part.oracle(k)
    ranks = LoopbackComm.group(world)
    try:
        def one(r):
            s = part.shards[r]
            res = [ranks[r].sharded_index_search(s["idx"], part.q, k, params=EXHAUSTIVE, filter_bitmap=s["flt"],
                                                 row_exists=s["rex"]) for _ in range(3)]
            return res, ranks[r].stats(), _lib.last_index_stats()

        out, errs = _run_ranks(world, one)
        _raise_first(errs)
        for r in range(world):
            res, cst, ist = out[r]
            for i, (ig, dg) in enumerate(res):
                bad = np.argwhere((ig != io) | (dg.view(np.uint32) != do.view(np.uint32)))
                assert len(bad) == 0, f"{name} rank {r} call {i}: {len(bad)} slots differ, first {tuple(bad[0])}"
            assert cst["fast_calls"] == 2, cst
            if name not in WRONG_GUESS:
                assert cst["redo_calls"] == 0, cst
            # mqvs_index_last_stats on a rank: its local search
            assert (ist["nq"], ist["k"], ist["nprobe"], ist["num_reorder"]) == (nq, k, 8, 4096), ist
        if name in WRONG_GUESS:
            # the case has power: with every base left at row_offset / granule
            # the merged result is NOT the oracle's
            per = [s["idx"].search(part.q, k, params=EXHAUSTIVE, filter_bitmap=s["flt"], row_exists=s["rex"])
                   for s in part.shards]
            ig, dg = merge_shards(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), metric)
            differ = int(((ig != io) | (dg.view(np.uint32) != do.view(np.uint32))).sum())
            print(f"{name}: {differ} of {io.size} slots differ with the bases left at row_offset / granule")
            assert differ > 0, f"{name}: no power, change SALT"
    finally:
        for c in ranks:
            c.free()
        part.free()


# ---- 3. partial probes == merge of the ranks' own searches (C1) ----------------------------------

PARTIAL = [
    # name,          metric,   filt, build,                 first_stage, row_ids
    ("l2",           "L2",     None, "nlist=16",            False,       False),
    ("cos_filter",   "Cosine", 0.7,  "nlist=16",            False,       False),
    ("l2_fp8",       "L2",     None, "nlist=16,plane=fp8",  False,       False),
    ("cos_first",    "Cosine", 0.7,  "nlist=16",            True,        False),
    ("l2_row_ids",   "L2",     None, "nlist=16",            False,       True),
]


@pytest.mark.parametrize("cfg", PARTIAL, ids=[c[0] for c in PARTIAL])
def test_loopback_partial_probes_equal_merge_of_shard_searches(mq, cfg):
    from myscaledb_amd.sharded import LoopbackComm
    from myscaledb_amd.vector_scan import merge_shards
    name, metric, filt, build, first, row_ids = cfg
    world, n, d, gran, k, nq = 4, 16384, 32, 1024, 20, 24
    part = Part(mq, "partial_" + name, world, n, d, nq, metric, 1, gran, filt, None, 0.0, True, build)
    ranks = LoopbackComm.group(world)
    try:
        if row_ids:
            rmap = (np.arange(n, dtype=np.uint64) * 3 + 7)
            for s in part.shards:
                s["idx"].set_row_ids_map(rmap)
        per = [s["idx"].search(part.q, k, params="nprobe=2", filter_bitmap=s["flt"], first_stage_only=first,
                               chunk_ord_base=s["base"]) for s in part.shards]
        exp = merge_shards(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), metric)
        if row_ids:
            assert (exp[0][exp[0] >= 0] % 3 == 1).all()

        def one(r):
            s = part.shards[r]
            return [ranks[r].sharded_index_search(s["idx"], part.q, k, params="nprobe=2", filter_bitmap=s["flt"],
                                                  first_stage_only=first) for _ in range(2)]

        out, errs = _run_ranks(world, one)
        _raise_first(errs)
        for r in range(world):
            for i, got in enumerate(out[r]):
                assert _same(got, exp), f"{name} rank {r} call {i}"
        assert ranks[0].stats()["fast_calls"] == 1
    finally:
        for c in ranks:
            c.free()
        part.free()


# ---- 4. one communicator, FLAT and index calls in turn -------------------------------------------

def test_loopback_mixed_kinds_on_one_communicator(mq):
    from myscaledb_amd.sharded import LoopbackComm
    world, n, d, gran, k, nq = 2, 8192, 16, 1024, 15, 6
    part = Part(mq, "mixed", world, n, d, nq, "Cosine", 1, gran)
    io, do = part.oracle(k)
    ranks = LoopbackComm.group(world)
    try:
        def one(r):
            s = part.shards[r]
            res = []
            for _ in range(2):
                res.append(ranks[r].sharded_search(s["seg"], part.q, k))
                res.append(ranks[r].sharded_index_search(s["idx"], part.q, k, params=EXHAUSTIVE))
            fast_mixed = ranks[r].stats()["fast_calls"]
            # a repeat of the last validated call (an index call) is fast; a FLAT call after it is not
            res.append(ranks[r].sharded_index_search(s["idx"], part.q, k, params=EXHAUSTIVE))
            res.append(ranks[r].sharded_search(s["seg"], part.q, k))
            return res, fast_mixed, ranks[r].stats()

        out, errs = _run_ranks(world, one)
        _raise_first(errs)
        for r in range(world):
            res, fast_mixed, st = out[r]
            for i, got in enumerate(res):
                assert _same(got, (io, do)), f"rank {r} call {i}"
            assert fast_mixed == 0 and st["fast_calls"] == 1 and st["redo_calls"] == 0, (fast_mixed, st)
    finally:
        for c in ranks:
            c.free()
        part.free()


# ---- 5. errors reach every rank, nothing hangs, the next call works ------------------------------

def test_loopback_index_errors_fail_everywhere_then_recover(mq):
    from myscaledb_amd import _lib
    from myscaledb_amd.sharded import LoopbackComm
    world, n, d, gran, k, nq = 2, 8192, 16, 1024, 10, 5
    part = Part(mq, "errors", world, n, d, nq, "L2", 1, gran)
    codes = np.random.default_rng(3).integers(0, 256, (4096, 16), dtype=np.uint8)
    bseg = mq.BinaryVectorScanSegment.from_codes(codes, granule=gran, row_offset=4096)
    bidx = mq.BinaryVectorIndex.build(bseg, params="nlist=8")
    io, do = part.oracle(k)
    ranks = LoopbackComm.group(world)

    def call(r, params, index=None, first=False):
        return ranks[r].sharded_index_search(index or part.shards[r]["idx"], part.q, k, params=params,
                                             first_stage_only=first)

    def good():
        out, errs = _run_ranks(world, lambda r: call(r, EXHAUSTIVE))
        assert errs == [None, None], errs
        for got in out:
            assert _same(got, (io, do))

    def fails(fn, status):
        _, errs = _run_ranks(world, fn)
        assert all(isinstance(e, _lib.MqvsError) for e in errs), errs
        assert [e.status for e in errs] == [status] * world, errs

    try:
        good()
        # the ranks disagree on params
        fails(lambda r: call(r, "nprobe=2" if r == 0 else "nprobe=4"), _lib.ERR_BAD_ARGUMENTS)
        good()
        good()  # (the fast path), then one rank repeats it and the other changes params
        fails(lambda r: call(r, EXHAUSTIVE if r == 0 else "nprobe=4"), _lib.ERR_BAD_ARGUMENTS)
        good()
        # nprobe above rank 1's nlist (rank 0's index has 16 lists): its local search fails
        idx16 = mq.VectorIndex.build(part.shards[0]["seg"], params="nlist=16")
        try:
            _, errs = _run_ranks(world, lambda r: call(r, "nprobe=12", idx16 if r == 0 else None))
            assert all(isinstance(e, _lib.MqvsError) for e in errs), errs
            assert "rank 1" in str(errs[0]) and "nprobe" in str(errs[1]), errs
            good()
        finally:
            idx16.free()
        # a binary index on one rank
        fails(lambda r: call(r, "nprobe=2", bidx if r == 1 else None), _lib.ERR_LOGICAL)
        good()
        # MQVS_F_FIRST_STAGE on one rank only
        fails(lambda r: call(r, EXHAUSTIVE, first=(r == 0)), _lib.ERR_BAD_ARGUMENTS)
        good()
    finally:
        for c in ranks:
            c.free()
        bidx.free()
        bseg.free()
        part.free()


# ---- 6. world 1 through RCCL --------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_rccl_world1_sharded_index_search_equals_index_search(mq):
    import torch
    import torch.distributed as dist
    from myscaledb_amd.sharded import RcclComm
    torch.cuda.set_device(0)
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    comm = seg = idx = None
    try:
        comm = RcclComm.from_process_group()
        assert (comm.nranks, comm.rank) == (1, 0)
        n, d, gran = 4096, 64, 1024
        seg = mq.VectorScanSegment.from_rows(O.generate(301, 2, 0, n, d), metric="Cosine", granule=gran)
        idx = mq.VectorIndex.build(seg, params="nlist=16")
        rex = mq.pack_bitmap(np.random.default_rng(5).random(n) >= 0.1)
        trex = torch.from_numpy(rex).cuda()
        for q, k, params in [(O.generate(302, 2, 0, 8, d), 30, "nprobe=3"),
                             (O.generate(303, 2, 0, 100, d), 50, "nprobe=2,num_reorder=200")]:
            exp = idx.search(q, k, params=params, row_exists=rex)
            tq = torch.from_numpy(q).cuda()
            for rep in range(3):
                ids, dist_ = comm.sharded_index_search(idx, tq, k, params=params, row_exists=trex)
                torch.cuda.synchronize()
                assert _same((ids.cpu().numpy(), dist_.cpu().numpy()), exp), rep
            assert _same(comm.sharded_index_search(idx, q, k, params=params, row_exists=rex), exp)
        st = comm.stats()
        # per case: 1 validated + 2 fast device calls, then 1 validated host call
        assert st["fast_calls"] == 4 and st["redo_calls"] == 0, st
    finally:
        for h in (comm, idx, seg):
            if h is not None:
                h.free()
        if own_group:
            dist.destroy_process_group()
