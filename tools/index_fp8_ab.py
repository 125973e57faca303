#!/usr/bin/env python3
"""The fp8 list plane (mqvs_index_build, plane=fp8) against the bf16 one, on
one GPU, at the bench's index configurations: 10M x 768 Cosine, nq 1000,
top-100, generator modes 2 and 3, the bench's nprobe settings.

Per distribution one part; the bf16 index is built with the default parameters
(as bench.py builds it), the fp8 index with the same parameters plus the list
count the bf16 build chose (a build of >= 2^20 rows picks nlist from timings of
the index it built, so the two formats could pick differently; with nlist
given the build is deterministic and the lists coincide, which is asserted).
Per nprobe setting: warm-up of both, per-stage kernel times from searches with
the timing events on, then `rounds` rounds of `steps` searches each,
alternating bf16 / fp8 (wall clock around work that ends in a device
synchronise).  One JSON line per (mode, setting), appended to --out:
QPS (median round, and every round), stage times, plane_bytes, reranked,
hbm_bytes and recall@10 against the FLAT truth, for both formats.

Asserted, because they follow from the layout: the fp8 scan streams half the
bf16 scan's bytes at equal probes, and the fp8 index's hbm_bytes is lower by
npos x dpad less the int16 scale array.  Scan time, QPS, recall and the number
of re-ranked candidates are measured and written down, not asserted.

    python tools/index_fp8_ab.py [--n 10000000] [--modes 2,3] [--out profiles/index_fp8/ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_BASE = 0x5EED0001  # bench.py's part
SETTINGS = {2: "nprobe=1;nprobe=2;nprobe=4;nprobe=8;nprobe=16", 3: "nprobe=1;nprobe=2;nprobe=4;nprobe=8"}  # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--modes", default="2,3")
    ap.add_argument("--steps", type=int, default=100, help="searches per timed round")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per format, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_fp8", "ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import myscaledb_amd as mq
    from myscaledb_amd.vector_index import last_index_stats
    from myscaledb_amd.vector_scan import generate_device, set_timing
    mq.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    n, d, nq, k = args.n, args.d, args.nq, args.k
    dpad = (d + 63) // 64 * 64

    for mode in [int(x) for x in args.modes.split(",")]:
        seg = mq.VectorScanSegment.generate(SEED_BASE, mode, n, d, args.metric, 8192)
        t0 = time.perf_counter()
        b16 = mq.VectorIndex.build(seg, "MSTG", "")
        build16 = time.perf_counter() - t0
        info16 = b16.info()
        t0 = time.perf_counter()
        f8 = mq.VectorIndex.build(seg, "MSTG", {"nlist": info16["nlist"], "plane": "fp8"})
        build8 = time.perf_counter() - t0
        info8 = f8.info()
        for a, b in zip(b16.lists(), f8.lists()):
            assert np.array_equal(a, b), "the two builds' lists differ"
        npos = info16["npos"]
        assert b16.plane() == {"format": 0, "plane_bytes": 2 * npos * dpad}
        assert f8.plane() == {"format": 1, "plane_bytes": npos * dpad + 2 * npos}
        assert info16["hbm_bytes"] - info8["hbm_bytes"] == npos * dpad - 2 * npos

        qi = torch.empty((nq, d), dtype=torch.float32, device="cuda")
        generate_device(SEED_BASE, mode, n, nq, d, qi)  # generator rows past the part
        gt = seg.search(qi, k)[0].cpu().numpy()
        ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dst = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        both = (("bf16", b16, info16), ("fp8", f8, info8))
        for sp in SETTINGS.get(mode, SETTINGS[2]).split(";"):
            rec = {"generator_mode": mode, "n": n, "d": d, "nq": nq, "k": k, "metric": args.metric, "search": sp,
                   "nlist": info16["nlist"], "npos": npos, "steps": args.steps, "rounds": args.rounds,
                   "build_s": {"bf16": round(build16, 2), "fp8_given_nlist": round(build8, 2)}}
            for name, idx, info in both:
                idx.search(qi, k, sp, out=(ids, dst))  # warm-up of the setting's shapes
                torch.cuda.synchronize()
                got = ids.cpu().numpy()
                set_timing(True)
                try:
                    sts = []
                    for _ in range(3):
                        idx.search(qi, k, sp, out=(ids, dst))
                        sts.append(last_index_stats())
                finally:
                    set_timing(False)
                st = min(sts, key=lambda x: x["total_ms"])
                rec[name] = {"recall_at_10": round(float(np.mean([len(set(got[i, :10]) & set(gt[i, :10]))
                                                                for i in range(nq)]) / 10), 4),
                             "kernel_ms": {x: round(st[x + "_ms"], 4) for x in ("coarse", "plan", "scan", "select",
                                                                                "rerank", "total")},
                             "plane_bytes": st["plane_bytes"], "reranked": st["reranked"],
                             "num_reorder": st["num_reorder"], "nprobe": st["nprobe"], "hbm_bytes": info["hbm_bytes"],
                             "ms_rounds": []}
            assert 2 * rec["fp8"]["plane_bytes"] == rec["bf16"]["plane_bytes"], rec
            for _ in range(args.rounds):
                for name, idx, _info in both:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        idx.search(qi, k, sp, out=(ids, dst))
                    torch.cuda.synchronize()
                    rec[name]["ms_rounds"].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
            for name, _idx, _info in both:
                ms = statistics.median(rec[name]["ms_rounds"])
                rec[name]["ms_per_search"] = round(ms, 4)
                rec[name]["qps"] = round(nq / (ms * 1e-3), 1)
            rec["fp8_over_bf16"] = {"qps": round(rec["fp8"]["qps"] / rec["bf16"]["qps"], 4),
                                    "scan_ms": round(rec["fp8"]["kernel_ms"]["scan"] /
                                                     max(rec["bf16"]["kernel_ms"]["scan"], 1e-9), 4),
                                    "hbm_bytes": round(info8["hbm_bytes"] / info16["hbm_bytes"], 4)}
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        b16.free()
        f8.free()
        seg.free()


if __name__ == "__main__":
    main()
