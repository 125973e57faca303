#!/usr/bin/env python
"""Times the i8 MFMA route of binary vectors against the popcount route, in
one process, and checks that both return the same bits.

search  a generated binary part (--rows x --bits, uniform random codes, on the
        device), k 100, Hamming and Jaccard, per nq: mqvs_search_binary with
        device pointers under mqvs_set_timing, route off (popcount scan,
        stats.path 3) and on (mqvs_set_binary_batch(1), stats.path 4)
        alternating within every round.  --routes popcount times the popcount
        route alone and touches no entry point of the MFMA route, so the same
        file runs against an earlier build of the library (the baseline of
        the unchanged route).  Times are the library's HIP-event
        times of the call (total_ms and the probe / main scan stages); the
        medians of three blocks of rounds in time order are kept, so the
        spread shows beside the median.  T pairs/s = rows x nq / total; the
        share is bit-MACs (rows x nq x bits) per second over the i8 issue rate
        of 1024 SIMDs x 1024 MAC per clock at --clock-mhz.
build   mqvs_index_build of a BINARYMSTG index with assign=valu and
        assign=mfma on the same part at the default nlist: info()["build_ms"]
        with the default 8 k-majority iterations and with kmeans_iters=0 (one
        assignment pass over every row plus the grouping: the two routes
        differ in the assign kernel only, so the difference of the two
        build_ms is the difference of the assign kernels), and that the two
        indexes hold the same centroids and lists.

One JSON line per measurement on stdout (and --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I8_MAC_PER_CLOCK = 1024 * 1024  # 256 CUs x 4 SIMDs x (16 x 16 x 64 MACs / 16 cycles)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def clocks():
    """The box's clock report (read only), or None."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else None
    except Exception:
        return None


def blocks(xs):
    """Medians of three blocks in time order, and the median of all."""
    n = len(xs) // 3
    b = [statistics.median(xs[i * n:(i + 1) * n]) for i in range(3)] if n else []
    return statistics.median(xs), b


def random_codes(torch, rows, nbytes, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (rows, nbytes), dtype=torch.uint8, device="cuda", generator=g)


def run_search(args):
    import torch
    import myscaledb_amd as mq
    from myscaledb_amd import _lib
    mq.init(0)
    mq.vector_scan.set_timing(True)
    k = args.k
    both = args.routes == ["popcount", "mfma"]
    for bits in args.bits:
        codes = random_codes(torch, args.rows, bits // 8, 1)
        seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
        for metric in ("Hamming", "Jaccard"):
            for nq in args.nq:
                q = random_codes(torch, nq, bits // 8, 2 + nq)
                out = {r: (torch.empty((nq, k), dtype=torch.int64, device="cuda"),
                           torch.empty((nq, k), dtype=torch.float32, device="cuda")) for r in args.routes}
                times = {r: {"total_ms": [], "probe_ms": [], "main_ms": []} for r in out}
                paths = {}
                for rnd in range(args.warmup + args.reps):
                    for route in args.routes:
                        if both:
                            prev = mq.set_binary_batch(1 if route == "mfma" else 0)
                        try:
                            seg.search(q, k, metric, out=out[route])
                            st = _lib.last_search_stats()
                        finally:
                            if both:
                                mq.set_binary_batch(prev)
                        paths[route] = st["path"]
                        if rnd >= args.warmup:
                            for f in times[route]:
                                times[route][f].append(st[f])
                same = None
                if both:
                    same = bool(torch.equal(out["popcount"][0], out["mfma"][0]) and
                                torch.equal(out["popcount"][1].view(torch.int32), out["mfma"][1].view(torch.int32)))
                rec = {"what": "search", "rows": args.rows, "bits": bits, "metric": metric, "nq": nq, "k": k,
                       "reps": args.reps, "same_bits": same, "paths": paths, "clock_mhz": args.clock_mhz}
                for route in out:
                    med, b = blocks(times[route]["total_ms"])
                    rec[route] = {
                        "total_ms": med, "block_medians_ms": b,
                        "probe_ms": statistics.median(times[route]["probe_ms"]),
                        "main_ms": statistics.median(times[route]["main_ms"]),
                        "tpairs_per_s": args.rows * nq / (med * 1e-3) / 1e12,
                    }
                if both:
                    m = rec["mfma"]["total_ms"] * 1e-3
                    rec["mfma"]["i8_share"] = args.rows * nq * bits / m / (I8_MAC_PER_CLOCK * args.clock_mhz * 1e6)
                    rec["speedup"] = rec["popcount"]["total_ms"] / rec["mfma"]["total_ms"]
                emit(rec, args.out)
        seg.free()
        del codes
    emit({"what": "clocks", "report": clocks()}, args.out)


def run_build(args):
    import numpy as np
    import torch
    import myscaledb_amd as mq
    mq.init(0)
    for bits in args.bits:
        for rows in args.build_rows:
            codes = random_codes(torch, rows, bits // 8, 3)
            seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
            rec = {"what": "build", "rows": rows, "bits": bits}
            for iters in (8, 0):
                kept = {}
                for assign in ("valu", "mfma"):
                    if assign == "valu" and rows > args.valu_max_rows and iters == 8:
                        rec[f"valu_iters{iters}"] = "not run (--valu-max-rows)"
                        continue
                    ms = []
                    for _ in range(args.build_reps):
                        idx = mq.BinaryVectorIndex.build(seg, params={"assign": assign, "kmeans_iters": iters})
                        info = idx.info()
                        ms.append(info["build_ms"])
                        if assign in kept or iters != 0:
                            idx.free()
                        else:
                            kept[assign] = idx
                    rec[f"{assign}_iters{iters}"] = {"build_ms": statistics.median(ms), "all_ms": ms,
                                                     "nlist": info["nlist"]}
                if len(kept) == 2:
                    a, b = kept["valu"], kept["mfma"]
                    la, lb = a.lists(), b.lists()
                    rec["same_index"] = bool(np.array_equal(a.centroids(), b.centroids()) and
                                             np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]))
                for idx in kept.values():
                    idx.free()
            emit(rec, args.out)
            seg.free()
            del codes
    emit({"what": "clocks", "report": clocks()}, args.out)


def ints(s):
    return [int(x) for x in s.split(",") if x]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["search", "build"])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--bits", type=ints, default=[256, 1024])
    ap.add_argument("--nq", type=ints, default=[8, 20, 64, 128, 1000])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clock-mhz", type=float, default=2400.0,
                    help="the clock the share of the i8 issue rate is stated at")
    ap.add_argument("--build-rows", type=ints, default=[1_000_000, 4_000_000])
    ap.add_argument("--build-reps", type=int, default=3)
    ap.add_argument("--valu-max-rows", type=int, default=1 << 62,
                    help="skip the 8-iteration assign=valu build above this many rows")
    ap.add_argument("--routes", type=lambda s: s.split(","), default=["popcount", "mfma"],
                    help="popcount,mfma (default) or popcount")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    run_search(args) if args.mode == "search" else run_build(args)


if __name__ == "__main__":
    main()
