#!/usr/bin/env python
"""Times mqvs_index_group_search_binary against what a caller could do before
it, for tables of many BINARYMSTG-indexed parts (random codes, default build),
and checks the bits.  The method is tools/part_group_bench.py's.

Per case (parts x rows, nq, metric; k 100, default nprobe) four variants, each
one call that ends with the merged result on the host side of a stream sync:
  a       the loop of synchronous mqvs_index_search_binary calls (host arrays)
          + mqvs_merge_shards
  b       the same loop with MQVS_F_DEVICE_PTRS | MQVS_F_ASYNC on one stream,
          the merge, then one mqvs_async_check
  c_host  mqvs_index_group_search_binary, host arrays as a
  c_dev   the same call, device arrays as b
The variants alternate within every round (3 warm-up, 33 timed); the rounds are
split into three blocks in time order and each block's median is kept, so the
spread of repeated runs shows beside the medians.  c's outputs must equal a's
bit for bit (equals_a).  A variant wins against another when its median is
below the other's by more than both variants' spreads.  The indexes of a case
are built once and serve every (metric, nq) of it.

One JSON line per measurement on stdout (and --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from part_group_bench import Table, ptr, time_variants, wins  # noqa: E402


class IndexTable(Table):
    """nparts binary segments with a default BINARYMSTG index each, their group,
    and everything the variants need; set_case() before run()."""

    def __init__(self, mq, nparts, rows, bits, k, seed=0x1D9C):
        from myscaledb_amd import _lib
        self.mq, self.lib, self._lib = mq, _lib.lib, _lib
        self.nparts, self.k, self.nbytes = nparts, k, bits // 8
        self.rng = np.random.default_rng(seed)
        t0 = time.perf_counter()
        self.segs = [mq.BinaryVectorScanSegment.from_codes(
            self.rng.integers(0, 256, (rows, self.nbytes), dtype=np.uint8), metric="Hamming", granule=8192)
            for _ in range(nparts)]
        self.idx = [mq.BinaryVectorIndex.build(s) for s in self.segs]
        self.build_s = time.perf_counter() - t0
        self.group = mq.BinaryIndexGroup(self.idx)
        self.nlist = self.idx[0].info()["nlist"]

    def set_case(self, metric, nq):
        import torch
        nparts, k = self.nparts, self.k
        self.nq, self.m, self.params = nq, self._lib.METRICS[metric], f"metric={metric}".encode()
        self.q = self.rng.integers(0, 256, (nq, self.nbytes), dtype=np.uint8)
        self.tq = torch.from_numpy(self.q).cuda()
        sh = (nparts, nq, k)
        self.h_ids, self.h_dist = np.empty(sh, np.int64), np.empty(sh, np.float32)
        self.t_ids = torch.empty(sh, dtype=torch.int64, device="cuda")
        self.t_dist = torch.empty(sh, dtype=torch.float32, device="cuda")
        self.out = {v: (np.empty((nq, k), np.int32), np.empty((nq, k), np.int64), np.empty((nq, k), np.float32))
                    for v in ("a", "c_host")}
        self.tout = {v: (torch.empty((nq, k), dtype=torch.int32, device="cuda"),
                         torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                         torch.empty((nq, k), dtype=torch.float32, device="cuda")) for v in ("b", "c_dev")}
        torch.cuda.synchronize()
        self.hp = [(ptr(self.h_ids[p]), ptr(self.h_dist[p])) for p in range(nparts)]
        self.tp = [(ptr(self.t_ids[p]), ptr(self.t_dist[p])) for p in range(nparts)]

    def run(self, v):
        L, _lib, nq, k, m, pr = self.lib, self._lib, self.nq, self.k, self.m, self.params
        if v == "a":
            qp = ptr(self.q)
            for ix, (ip, dp) in zip(self.idx, self.hp):
                _lib.check(L.mqvs_index_search_binary(ix._h, qp, nq, k, pr, None, None, ip, dp, 0, None))
            o = self.out["a"]
            _lib.check(L.mqvs_merge_shards(self.nparts, nq, k, m, ptr(self.h_ids), ptr(self.h_dist), ptr(o[1]),
                                           ptr(o[2]), _lib.F_PART_MERGE, None))
        elif v == "b":
            qp = ptr(self.tq)
            fl = _lib.F_DEVICE_PTRS | _lib.F_ASYNC
            for ix, (ip, dp) in zip(self.idx, self.tp):
                _lib.check(L.mqvs_index_search_binary(ix._h, qp, nq, k, pr, None, None, ip, dp, fl, None))
            o = self.tout["b"]
            _lib.check(L.mqvs_merge_shards(self.nparts, nq, k, m, ptr(self.t_ids), ptr(self.t_dist), ptr(o[1]),
                                           ptr(o[2]), fl | _lib.F_PART_MERGE, None))
            _lib.check(L.mqvs_async_check(None))
        elif v == "c_host":
            o = self.out["c_host"]
            _lib.check(L.mqvs_index_group_search_binary(self.group._h, ptr(self.q), nq, k, pr, None, None, ptr(o[0]),
                                                        ptr(o[1]), ptr(o[2]), 0, None))
        else:
            o = self.tout["c_dev"]
            _lib.check(L.mqvs_index_group_search_binary(self.group._h, ptr(self.tq), nq, k, pr, None, None, ptr(o[0]),
                                                        ptr(o[1]), ptr(o[2]), _lib.F_DEVICE_PTRS, None))

    def free(self):
        self.group.free()
        for ix in self.idx:
            ix.free()
        for s in self.segs:
            s.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="8x1048576,32x262144,128x65536", help="PARTSxROWS,...")
    ap.add_argument("--code-bits", type=int, default=256, help="code width in bits (a multiple of 8)")
    ap.add_argument("--nqs", default="1,16,128")
    ap.add_argument("--metrics", default="Hamming,Jaccard")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=33)
    ap.add_argument("--variants", default="a,b,c_host,c_dev")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import myscaledb_amd as mq
    from myscaledb_amd.index_group import last_stats
    mq.init(0)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    variants = [v for v in args.variants.split(",") if v]
    for case in [c for c in args.cases.split(",") if c]:
        nparts, rows = (int(x) for x in case.split("x"))
        tb = IndexTable(mq, nparts, rows, args.code_bits, args.k)
        try:
            for metric in args.metrics.split(","):
                for nq in (int(x) for x in args.nqs.split(",")):
                    tb.set_case(metric, nq)
                    res = time_variants(tb.run, variants, args.warmup, args.rounds)
                    same = None
                    if "a" in variants:
                        ia, da = tb.results("a")
                        same = {}
                        for v in variants:
                            if v == "a":
                                continue
                            iv, dv = tb.results(v)
                            same[v] = bool(np.array_equal(ia, iv) and
                                           np.array_equal(da.view(np.uint32), dv.view(np.uint32)))
                    st = None
                    if any(v.startswith("c") for v in variants):
                        tb.run([v for v in variants if v.startswith("c")][0])
                        st = last_stats()
                    rec = dict(kind="case", parts=nparts, rows=rows, bits=args.code_bits, nlist=tb.nlist, nq=nq,
                               k=args.k, metric=metric, build_s=round(tb.build_s, 2), times=res, equals_a=same,
                               group_stats=st)
                    if "b" in res and "c_dev" in res:
                        rec["c_dev_wins"] = dict(b=wins(res, "c_dev", "b"))
                        rec["b_wins"] = dict(c_dev=wins(res, "b", "c_dev"))
                    emit(rec)
                    if same and not all(same.values()):
                        raise SystemExit(f"outputs differ from variant a: {same}")
        finally:
            tb.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
