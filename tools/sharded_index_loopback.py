#!/usr/bin/env python3
"""mqvs_sharded_index_search on ONE GPU: what the protocol costs on top of
mqvs_index_search (world 1), and a rehearsal of 2 / 4 / 8 row-range shards
with one index each over loopback ranks (a thread per rank, all on the same
device -- NOT a scaling curve: the ranks share the GPU; RCCL over more than
one GPU is not measured here).

Workload: the bench's index setting on the hard distribution -- 10M x 768
Cosine, generator mode 3, nq 1000, top-100, nprobe=1, default num_reorder.

World 1: `rounds` rounds of `steps` calls each, alternating mqvs_index_search
and mqvs_sharded_index_search on its one-sync fast path (wall clock around
work that ends in a device synchronise); the difference of the medians is
the protocol's cost (header, two list gathers, merge, one host sync).
World N > 1: every rank builds the index of its own shard with the default
parameters; per round all ranks make `steps` calls together; wall time per
call, the communicator's fast_calls and recall@10 against the FLAT truth
(mqvs_sharded_search over the same shards).  One JSON line per world,
appended to --out.

--index-only measures mqvs_index_search alone; with --root it measures
another checkout's library (the parent commit's, to show the call did not
move), labelled by --label.

    python tools/sharded_index_loopback.py [--world 1,2,4,8] [--out profiles/sharded_index/loopback.jsonl]
    python tools/sharded_index_loopback.py --index-only --root ../parent --label parent
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_BASE = 0x5EED0001  # bench.py's part


def recall_at_10(got, gt):
    return round(sum(len(set(got[i, :10]) & set(gt[i, :10])) for i in range(len(gt))) / (10.0 * len(gt)), 4)


def timed(fn, steps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default="1,2,4,8")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--mode", type=int, default=3)
    ap.add_argument("--granule", type=int, default=8192)
    ap.add_argument("--search", default="nprobe=1")
    ap.add_argument("--steps", type=int, default=50, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--index-only", action="store_true", help="time mqvs_index_search only")
    ap.add_argument("--root", default=ROOT, help="the checkout whose myscaledb_amd is measured")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_index", "loopback.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import myscaledb_amd as mq
    from myscaledb_amd.sharded import shard_rows
    from myscaledb_amd.vector_scan import generate_device
    mq.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    n, d, nq, k, sp = args.n, args.d, args.nq, args.k, args.search
    qi = torch.empty((nq, d), dtype=torch.float32, device="cuda")
    generate_device(SEED_BASE, args.mode, n, nq, d, qi)  # generator rows past the part
    torch.cuda.synchronize()
    base = {"label": args.label, "generator_mode": args.mode, "n": n, "d": d, "nq": nq, "k": k,
            "metric": args.metric, "search": sp, "steps": args.steps, "rounds": args.rounds}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    def bufs():
        return (torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                torch.empty((nq, k), dtype=torch.float32, device="cuda"))

    for world in [int(x) for x in args.world.split(",")]:
        if world == 1 or args.index_only:
            seg = mq.VectorScanSegment.generate(SEED_BASE, args.mode, n, d, args.metric, args.granule)
            idx = mq.VectorIndex.build(seg, "MSTG", "")
            out = bufs()
            gt = seg.search(qi, k)[0].cpu().numpy()
            idx.search(qi, k, sp, out=out)
            torch.cuda.synchronize()
            rec = dict(base, world=1, nlist=idx.info()["nlist"], recall_at_10=recall_at_10(out[0].cpu().numpy(), gt),
                       index_search_ms_rounds=[])
            legs = [("index_search", lambda: idx.search(qi, k, sp, out=out))]
            comm = None
            if not args.index_only:
                from myscaledb_amd.sharded import LoopbackComm
                comm = LoopbackComm.group(1)[0]
                sout = bufs()
                for _ in range(2):  # the validated call, then a first fast one
                    comm.sharded_index_search(idx, qi, k, sp, out=sout)
                torch.cuda.synchronize()
                assert torch.equal(sout[0], out[0]) and torch.equal(sout[1].view(torch.int32), out[1].view(torch.int32))
                legs.append(("sharded_index_search", lambda: comm.sharded_index_search(idx, qi, k, sp, out=sout)))
                rec["sharded_index_search_ms_rounds"] = []
            for _ in range(args.rounds):
                for name, fn in legs:
                    rec[name + "_ms_rounds"].append(round(timed(fn, args.steps, torch.cuda.synchronize), 4))
            for name, _fn in legs:
                rec[name + "_ms"] = round(statistics.median(rec[name + "_ms_rounds"]), 4)
            if comm is not None:
                rec["protocol_ms"] = round(rec["sharded_index_search_ms"] - rec["index_search_ms"], 4)
                rec.update(comm.stats())
                comm.free()
            emit(rec)
            idx.free()
            seg.free()
            if args.index_only:
                break
            continue

        from myscaledb_amd.sharded import LoopbackComm
        ranks = LoopbackComm.group(world)
        shards = []
        t0 = time.perf_counter()
        for r in range(world):
            r0, r1 = shard_rows(n, args.granule, r, world)
            seg = mq.VectorScanSegment.generate(SEED_BASE, args.mode, r1 - r0, d, args.metric, args.granule,
                                                row_offset=r0)
            shards.append((seg, mq.VectorIndex.build(seg, "MSTG", ""), bufs(), torch.cuda.Stream()))
        build_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        gate = threading.Barrier(world + 1)
        errs = []

        def rank_main(r, plan):
            seg, idx, out, st = shards[r]
            try:
                for kind, steps in plan:
                    gate.wait()
                    for _ in range(steps):
                        if kind == "flat":
                            ranks[r].sharded_search(seg, qi, k, out=out, stream=st.cuda_stream)
                        else:
                            ranks[r].sharded_index_search(idx, qi, k, sp, out=out, stream=st.cuda_stream)
                    gate.wait()
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
                gate.abort()

        # FLAT truth, a warm-up of the index call (validated, then fast), the timed rounds
        plan = [("flat", 1), ("index", 2)] + [("index", args.steps)] * args.rounds
        th = [threading.Thread(target=rank_main, args=(r, plan)) for r in range(world)]
        for t in th:
            t.start()
        rec = dict(base, world=world, nlist=[s[1].info()["nlist"] for s in shards], build_s=round(build_s, 2),
                   ms_rounds=[], note="one-GPU rehearsal: the ranks share the device")
        gt = None
        try:
            for i, (kind, steps) in enumerate(plan):
                gate.wait()
                t0 = time.perf_counter()
                gate.wait()  # every rank's last call has synchronised its stream
                ms = (time.perf_counter() - t0) * 1e3 / steps
                if i == 0:
                    gt = shards[0][2][0].cpu().numpy()
                elif i == 1:
                    rec["recall_at_10"] = recall_at_10(shards[0][2][0].cpu().numpy(), gt)
                else:
                    rec["ms_rounds"].append(round(ms, 4))
        except threading.BrokenBarrierError:
            pass
        for t in th:
            t.join()
        if errs:
            raise errs[0]
        rec["ms_per_call"] = round(statistics.median(rec["ms_rounds"]), 4)
        rec["qps"] = round(nq / (rec["ms_per_call"] * 1e-3), 1)
        rec.update(ranks[0].stats())
        emit(rec)
        for seg, idx, _o, _s in shards:
            idx.free()
            seg.free()
        for c in ranks:
            c.free()


if __name__ == "__main__":
    main()
