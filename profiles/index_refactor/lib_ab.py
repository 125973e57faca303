"""One library's share of a parent / branch comparison of the index search, at
the bench's index configurations (10M x 768 Cosine, nq 1000, top-100, generator
modes 2 and 3, nprobe 1 and the bench's largest setting, bf16 and fp8 planes).

A process loads one libmqvs.so (the tree it is run from), so the two libraries
are alternated as processes: run this script in the parent's tree and in the
branch's, in turn, several times; every run appends one JSON line per (mode,
plane, setting) with its tag.  The list counts are given (the ones the default
build chooses for these parts), so every process searches the same lists.  Per
setting: warm-up, scan_ms from searches with the timing events on (the least
of 5), then `rounds` rounds of `steps` searches each, wall clock around work
that ends in a device synchronise.

    python profiles/index_refactor/lib_ab.py <tag> <out.jsonl> [--modes 2,3] [--steps 50] [--rounds 3]
    python profiles/index_refactor/lib_ab.py --reduce <out.jsonl>
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEED_BASE = 0x5EED0001  # bench.py's part
NLIST = {2: 4883, 3: 39063}  # the default build's choice for 10M rows of these modes
NPROBES = {2: (1, 16), 3: (1, 8)}  # bench.py's first and largest setting


def measure(args):
    import torch
    import myscaledb_amd as mq
    from myscaledb_amd.vector_index import last_index_stats
    from myscaledb_amd.vector_scan import generate_device, set_timing
    mq.init(0)
    n, d, nq, k = args.n, 768, 1000, 100
    for mode in [int(x) for x in args.modes.split(",")]:
        seg = mq.VectorScanSegment.generate(SEED_BASE, mode, n, d, "Cosine", 8192)
        qi = torch.empty((nq, d), dtype=torch.float32, device="cuda")
        generate_device(SEED_BASE, mode, n, nq, d, qi)  # generator rows past the part
        ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dst = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        for plane in ("bf16", "fp8"):
            idx = mq.VectorIndex.build(seg, "MSTG", {"nlist": NLIST[mode], "plane": plane})
            for nprobe in NPROBES[mode]:
                sp = f"nprobe={nprobe}"
                idx.search(qi, k, sp, out=(ids, dst))
                torch.cuda.synchronize()
                set_timing(True)
                try:
                    scan = []
                    for _ in range(5):
                        idx.search(qi, k, sp, out=(ids, dst))
                        scan.append(last_index_stats()["scan_ms"])
                finally:
                    set_timing(False)
                rounds = []
                for _ in range(args.rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        idx.search(qi, k, sp, out=(ids, dst))
                    torch.cuda.synchronize()
                    rounds.append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
                rec = {"tag": args.tag, "generator_mode": mode, "plane": plane, "search": sp, "n": n,
                       "scan_ms": round(min(scan), 4), "ms_rounds": rounds,
                       "qps_rounds": [round(nq / (ms * 1e-3)) for ms in rounds]}
                line = json.dumps(rec)
                print(line, flush=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            idx.free()
        seg.free()


def reduce(path):
    """Per (mode, plane, setting): the parent's range over all its rounds and the branch's median."""
    rows = [json.loads(x) for x in open(path) if x.strip()]
    keys = sorted({(r["generator_mode"], r["plane"], r["search"]) for r in rows})
    print("| mode | plane | search | parent scan ms (min..max) | branch scan ms (median) | parent QPS (min..max, median)"
          " | branch QPS (median) | inside |")
    print("|---|---|---|---|---|---|---|---|")
    for key in keys:
        sel = {t: [r for r in rows if (r["generator_mode"], r["plane"], r["search"]) == key and r["tag"] == t]
               for t in ("parent", "branch")}
        ps = [r["scan_ms"] for r in sel["parent"]]
        bs = statistics.median(r["scan_ms"] for r in sel["branch"])
        pq = [q for r in sel["parent"] for q in r["qps_rounds"]]
        bq = statistics.median(q for r in sel["branch"] for q in r["qps_rounds"])
        ok = ("scan " + ("yes" if min(ps) <= bs <= max(ps) else "faster" if bs < min(ps) else "SLOWER") +
              ", QPS " + ("yes" if min(pq) <= bq <= max(pq) else "faster" if bq > max(pq) else "SLOWER"))
        print(f"| {key[0]} | {key[1]} | {key[2]} | {min(ps):.4f}..{max(ps):.4f} | {bs:.4f} | "
              f"{min(pq)}..{max(pq)}, {statistics.median(pq):.0f} | {bq:.0f} | {ok} |")


if __name__ == "__main__":
    if sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    else:
        ap = argparse.ArgumentParser()
        ap.add_argument("tag")
        ap.add_argument("out")
        ap.add_argument("--n", type=int, default=10_000_000)
        ap.add_argument("--modes", default="2,3")
        ap.add_argument("--steps", type=int, default=50)
        ap.add_argument("--rounds", type=int, default=3)
        measure(ap.parse_args())
