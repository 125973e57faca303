#!/usr/bin/env python3
"""What loading a saved index costs against building it, on one GPU: for the
bench's index part (10M x 768 Cosine, generator mode 3, default parameters)
and the 100M x 256-bit binary shape of profiles/r01/binary, one JSON line each
with the build, save and load times and the blob size.  One process, one pass,
nothing repeated: each step is timed once by the wall clock around the call
(every call is synchronous), and the library's own device time of the build
and of the load (mqvs_index_info.build_ms) is reported beside it.  A search of
64 queries is compared between the built and the loaded index.

    python tools/index_load_time.py [--shapes float,binary] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_BASE = 0x5EED0001  # bench.py's part


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def measure(mq, seg, cls, index_type, queries, label, extra):
    import numpy as np
    idx, build_wall = timed(lambda: cls.build(seg, index_type))
    info = idx.info()
    expect = idx.search(queries, 10)
    blob, save_wall = timed(idx.save)
    idx.free()
    ld, load_wall = timed(lambda: cls.load(seg, blob))
    linfo = ld.info()
    got = ld.search(queries, 10)
    same = bool(np.array_equal(expect[0], got[0]) and
                np.array_equal(expect[1].view(np.uint32), got[1].view(np.uint32)))
    same = same and all(info[f] == linfo[f] for f in ("nlist", "npos", "max_list", "rows_indexed", "hbm_bytes"))
    ld.free()
    return {"shape": label, **extra, "nlist": info["nlist"], "index_hbm_bytes": info["hbm_bytes"],
            "blob_bytes": len(blob), "np95": mq.index_blob_info(blob)["np95"],
            "build_wall_ms": round(build_wall, 1), "build_ms": round(info["build_ms"], 1),
            "save_wall_ms": round(save_wall, 1), "load_wall_ms": round(load_wall, 1),
            "load_device_ms": round(linfo["build_ms"], 1),
            "build_over_load": round(build_wall / load_wall, 1), "loaded_equals_built": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="float,binary")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--binary-n", type=int, default=100_000_000)
    ap.add_argument("--bits", type=int, default=256)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    import myscaledb_amd as mq
    from oracle import oracle as O
    mq.init(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for shape in args.shapes.split(","):
        if shape == "float":
            seg = mq.VectorScanSegment.generate(SEED_BASE, 3, args.n, args.d, "Cosine", 8192)
            q = O.generate(SEED_BASE, 3, args.n, 64, args.d)  # generator rows past the part
            emit(measure(mq, seg, mq.VectorIndex, "MSTG", q, f"{args.n} x {args.d} Cosine, generator mode 3",
                         {"n": args.n, "d": args.d}))
            seg.free()
        elif shape == "binary":
            nb = args.bits // 8
            g = torch.Generator(device="cuda").manual_seed(1)
            codes = torch.randint(0, 256, (args.binary_n, nb), dtype=torch.uint8, device="cuda", generator=g)
            seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
            q = codes[:: args.binary_n // 64][:64].cpu().numpy().copy()
            q[:, 0] ^= 0x5A
            del codes
            torch.cuda.empty_cache()
            emit(measure(mq, seg, mq.BinaryVectorIndex, "BINARYMSTG", q,
                         f"{args.binary_n} x {args.bits} bits Hamming, random codes",
                         {"n": args.binary_n, "bits": args.bits}))
            seg.free()
        else:
            raise SystemExit(f"unknown shape `{shape}`")


if __name__ == "__main__":
    main()
