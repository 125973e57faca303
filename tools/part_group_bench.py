#!/usr/bin/env python
"""Times mqvs_part_group_search against what a caller could do before it, for
tables of many small parts (generated segments), and checks the bits.

Per case (parts x rows x d, nq, metric; k 100) three variants, each one call
that ends with the merged result on the host side of a stream sync:
  a  the loop of synchronous mqvs_search calls (host arrays) + mqvs_merge_shards
  b  the same loop with MQVS_F_DEVICE_PTRS | MQVS_F_ASYNC on one stream, the
     merge, then one mqvs_async_check
  c  mqvs_part_group_search (c_host: host arrays as a, c_dev: device arrays as b)
The variants alternate within every round; the rounds are split into three
blocks in time order and each block's median is kept, so the spread of
repeated runs shows beside the medians.  c's outputs must equal a's bit for
bit.  --limit-sweep times groups of 8 equal parts with the fused route on and
off, per part size: where the per-part route becomes faster is where the
default of mqvs_set_part_group_rows belongs.

--batch is the same method for batches (nq >= 20; default nq 20, 128, 1000)
and the fused batch route (mqvs_set_part_group_batch), device arrays
throughout:
  b      as above
  c_off  mqvs_part_group_search with the batch route off: every part looped
         inside the call
  c_on   the same call with the batch route on
a runs once, untimed, and the outputs of c_off and c_on must equal it bit for
bit.  Each record carries, per variant, the spread of the three block medians
and whether c_on wins against b and against c_off: its median is below the
other's by more than both spreads.  With --batch, --limit-sweep times c_on
against c_off for groups of 8 equal parts per part size and nq.

--binary is the same method (variants a, b, c_host, c_dev and --limit-sweep)
for binary parts: generated FixedString codes of --code-bits bits (default
256), mqvs_search_binary per part against mqvs_part_group_search_binary,
Hamming and Jaccard, default nq 1, 16, 128; the limit sweep sets
mqvs_set_part_group_binary_rows.  Each record carries whether c_dev wins
against b: its median is below b's by more than both variants' spreads.

One JSON line per measurement on stdout (and --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def ptr(a):
    if a is None:
        return None
    if type(a).__module__.startswith("torch"):
        return ctypes.c_void_p(a.data_ptr())
    return a.ctypes.data_as(ctypes.c_void_p)


class Table:
    """nparts generated segments + everything the three variants need, with
    the pointers taken once (the timed loops are library calls only)."""

    def __init__(self, mq, nparts, rows, d, metric, nq, k, seed=0xBE9C):
        import torch
        from myscaledb_amd import _lib
        self.mq, self.lib, self._lib = mq, _lib.lib, _lib
        self.nparts, self.nq, self.k, self.m = nparts, nq, k, _lib.METRICS[metric]
        self.make(mq, nparts, rows, d, metric, nq, seed)
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

    def make(self, mq, nparts, rows, d, metric, nq, seed):
        """the segments, their group, the host queries and the two search calls"""
        self.segs = [mq.VectorScanSegment.generate(seed + p, 1, rows, d, metric=metric, granule=8192)
                     for p in range(nparts)]
        self.group = mq.PartGroup(self.segs)
        self.q = np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)
        self.search, self.group_search = self.lib.mqvs_search, self.lib.mqvs_part_group_search

    def run(self, v):
        L, _lib, nq, k, m = self.lib, self._lib, self.nq, self.k, self.m
        if v == "a":
            qp = ptr(self.q)
            for s, (ip, dp) in zip(self.segs, self.hp):
                _lib.check(self.search(s._h, qp, nq, k, m, None, None, ip, dp, 0, None))
            o = self.out["a"]
            _lib.check(L.mqvs_merge_shards(self.nparts, nq, k, m, ptr(self.h_ids), ptr(self.h_dist), ptr(o[1]),
                                           ptr(o[2]), _lib.F_PART_MERGE, None))
        elif v == "b":
            qp = ptr(self.tq)
            fl = _lib.F_DEVICE_PTRS | _lib.F_ASYNC
            for s, (ip, dp) in zip(self.segs, self.tp):
                _lib.check(self.search(s._h, qp, nq, k, m, None, None, ip, dp, fl, None))
            o = self.tout["b"]
            _lib.check(L.mqvs_merge_shards(self.nparts, nq, k, m, ptr(self.t_ids), ptr(self.t_dist), ptr(o[1]),
                                           ptr(o[2]), fl | _lib.F_PART_MERGE, None))
            _lib.check(L.mqvs_async_check(None))
        elif v == "c_host":
            o = self.out["c_host"]
            _lib.check(self.group_search(self.group._h, ptr(self.q), nq, k, m, None, None, ptr(o[0]), ptr(o[1]),
                                         ptr(o[2]), 0, None))
        else:
            o = self.tout["c_dev"]
            _lib.check(self.group_search(self.group._h, ptr(self.tq), nq, k, m, None, None, ptr(o[0]), ptr(o[1]),
                                         ptr(o[2]), _lib.F_DEVICE_PTRS, None))

    def results(self, v):
        if v in self.out:
            return self.out[v][1], self.out[v][2]
        return self.tout[v][1].cpu().numpy(), self.tout[v][2].cpu().numpy()

    def free(self):
        self.group.free()
        for s in self.segs:
            s.free()


class BinaryTable(Table):
    """the same over generated binary parts: d is the code width in bits"""

    def make(self, mq, nparts, rows, d, metric, nq, seed):
        rng = np.random.default_rng(seed)
        self.segs = [mq.BinaryVectorScanSegment.from_codes(rng.integers(0, 256, (rows, d // 8), dtype=np.uint8),
                                                           metric=metric, granule=8192) for _ in range(nparts)]
        self.group = mq.BinaryPartGroup(self.segs)
        self.q = rng.integers(0, 256, (nq, d // 8), dtype=np.uint8)
        self.search, self.group_search = self.lib.mqvs_search_binary, self.lib.mqvs_part_group_search_binary


def time_variants(run, variants, warmup, rounds):
    """alternating rounds; per variant the median, the three block medians, min and max (ms)"""
    for _ in range(warmup):
        for v in variants:
            run(v)
    t = {v: [] for v in variants}
    for _ in range(rounds):
        for v in variants:
            t0 = time.perf_counter()
            run(v)
            t[v].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for v, x in t.items():
        b = max(1, len(x) // 3)
        blocks = [statistics.median(x[i:i + b]) for i in range(0, b * 3, b) if x[i:i + b]]
        out[v] = dict(median_ms=statistics.median(x), block_medians_ms=blocks, spread_ms=max(blocks) - min(blocks),
                      min_ms=min(x), max_ms=max(x), rounds=len(x))
    return out


def wins(res, v, other):
    """v's median is below other's by more than both variants' spread"""
    return bool(res[other]["median_ms"] - res[v]["median_ms"] > max(res[v]["spread_ms"], res[other]["spread_ms"]))


def batch_mode(args, mq, emit):
    """--batch: b, c_off and c_on per case, then the limit sweep (c_on against c_off)"""
    from myscaledb_amd.part_group import last_stats, part_group_batch, set_part_group_batch
    prev = part_group_batch()
    nqs = [int(x) for x in (args.nqs if args.nqs != "1,16" else "20,128,1000").split(",")]

    def runner(tb):
        def run(v):
            if v in ("c_off", "c_on"):
                set_part_group_batch((1 << 24) if v == "c_on" else 0)
                tb.run("c_dev")
            else:
                tb.run(v)
        return run

    def same_as_a(tb, run):
        run("a")
        ia, da = tb.results("a")
        same, stats = {}, {}
        for v in ("c_off", "c_on"):
            run(v)
            iv, dv = tb.results("c_dev")
            same[v] = bool(np.array_equal(ia, iv) and np.array_equal(da.view(np.uint32), dv.view(np.uint32)))
            stats[v] = last_stats()
        return same, stats

    try:
        for case in [c for c in args.cases.split(",") if c]:
            nparts, rows = (int(x) for x in case.split("x"))
            for metric in args.metrics.split(","):
                for nq in nqs:
                    tb = Table(mq, nparts, rows, args.dim, metric, nq, args.k)
                    try:
                        run = runner(tb)
                        res = time_variants(run, ["b", "c_off", "c_on"], args.warmup, args.rounds)
                        same, stats = same_as_a(tb, run)
                        emit(dict(kind="batch_case", parts=nparts, rows=rows, d=args.dim, nq=nq, k=args.k,
                                  metric=metric, times=res, equals_a=same, group_stats=stats,
                                  c_on_wins=dict(b=wins(res, "c_on", "b"), c_off=wins(res, "c_on", "c_off"))))
                        if not all(same.values()):
                            raise SystemExit(f"outputs differ from variant a: {same}")
                    finally:
                        tb.free()
        for rows in [int(x) for x in args.limit_sweep.split(",") if x]:
            for metric in args.metrics.split(","):
                for nq in nqs:
                    tb = Table(mq, 8, rows, args.dim, metric, nq, args.k)
                    try:
                        run = runner(tb)
                        res = time_variants(run, ["c_off", "c_on"], args.warmup, args.rounds)
                        same, stats = same_as_a(tb, run)
                        emit(dict(kind="batch_limit", parts=8, rows=rows, d=args.dim, nq=nq, k=args.k, metric=metric,
                                  times=res, equals_a=same, group_stats=stats,
                                  c_on_wins=dict(c_off=wins(res, "c_on", "c_off"))))
                        if not all(same.values()):
                            raise SystemExit(f"outputs differ from variant a: {same}")
                    finally:
                        tb.free()
    finally:
        set_part_group_batch(*prev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="64x8192,256x1000", help="PARTSxROWS,... (d from --dim)")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nqs", default="1,16")
    ap.add_argument("--metrics", default="L2,Cosine")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=33)
    ap.add_argument("--variants", default="a,b,c_host,c_dev")
    ap.add_argument("--limit-sweep", default="", help="part sizes ROWS,... of the row-limit sweep (8 parts each)")
    ap.add_argument("--batch", action="store_true", help="the batch route: b, c_off, c_on at nq >= 20 (see above)")
    ap.add_argument("--binary", action="store_true", help="binary parts (see above)")
    ap.add_argument("--code-bits", type=int, default=256, help="--binary: code width in bits (a multiple of 8)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import myscaledb_amd as mq
    from myscaledb_amd.part_group import last_stats, set_part_group_binary_rows, set_part_group_rows
    mq.init(0)
    make_table, set_rows, sweep_metrics = Table, set_part_group_rows, ["L2"]
    if args.binary:
        if args.batch:
            raise SystemExit("--binary has no batch route: one fused route serves every nq")
        make_table, set_rows, args.dim = BinaryTable, set_part_group_binary_rows, args.code_bits
        if args.metrics == "L2,Cosine":
            args.metrics = "Hamming,Jaccard"
        if args.nqs == "1,16":
            args.nqs = "1,16,128"
        sweep_metrics = args.metrics.split(",")
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if args.batch:
        batch_mode(args, mq, emit)
        if sink:
            sink.close()
        return

    variants = [v for v in args.variants.split(",") if v]
    for case in [c for c in args.cases.split(",") if c]:
        nparts, rows = (int(x) for x in case.split("x"))
        for metric in args.metrics.split(","):
            for nq in (int(x) for x in args.nqs.split(",")):
                tb = make_table(mq, nparts, rows, args.dim, metric, nq, args.k)
                try:
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
                    rec = dict(kind="case", parts=nparts, rows=rows, d=args.dim, nq=nq, k=args.k, metric=metric,
                               times=res, equals_a=same, group_stats=st)
                    if args.binary and "b" in res and "c_dev" in res:
                        rec["c_dev_wins"] = dict(b=wins(res, "c_dev", "b"))
                    emit(rec)
                    if same and not all(same.values()):
                        raise SystemExit(f"outputs differ from variant a: {same}")
                finally:
                    tb.free()

    for rows, metric in [(int(x), mt) for x in args.limit_sweep.split(",") if x for mt in sweep_metrics]:
        for nq in (int(x) for x in args.nqs.split(",")):
            tb = make_table(mq, 8, rows, args.dim, metric, nq, args.k)
            prev = set_rows(0)
            try:
                def run(v):
                    set_rows(rows if v == "fused" else 1)
                    tb.run("c_dev")
                res = time_variants(run, ["fused", "per_part"], args.warmup, args.rounds)
                rec = dict(kind="limit", parts=8, rows=rows, d=args.dim, nq=nq, k=args.k, metric=metric, times=res)
                if args.binary:
                    rec["fused_wins"] = wins(res, "fused", "per_part")
                emit(rec)
            finally:
                set_rows(prev)
                tb.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
