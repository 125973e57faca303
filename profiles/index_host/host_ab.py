"""One library's share of a parent / branch comparison of the index host code:
binary index search QPS at nq 1 and 1000 (random 256-bit codes generated on
the device with seed 1, as tools/binary_sweep.py makes its part; 10M rows,
nlist 4096, default nprobe, top-100, device pointers, synchronous), and
build_ms of that binary index and of a float index (1M x 128 L2, generator
mode 3, nlist 1024).  A process loads the libmqvs.so of the tree the script
is run from, so the two libraries are alternated as processes; every run
appends JSON lines with its tag.

    python profiles/index_host/host_ab.py <tag> <out.jsonl>
    python profiles/index_host/host_ab.py --reduce <out.jsonl>
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def measure(tag, out):
    import torch
    import myscaledb_amd as mq
    mq.init(0)

    def emit(rec):
        line = json.dumps({"tag": tag, **rec})
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")

    n, nb, k = 10_000_000, 32, 100
    g = torch.Generator(device="cuda").manual_seed(1)
    codes = torch.randint(0, 256, (n, nb), dtype=torch.uint8, device="cuda", generator=g)
    seg = mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
    del codes
    idx = mq.BinaryVectorIndex.build(seg, "BINARYMSTG", "nlist=4096")
    emit({"what": "binary build_ms", "n": n, "value": round(idx.info()["build_ms"], 2)})
    for nq, steps in ((1, 500), (1000, 20)):
        q = torch.randint(0, 256, (nq, nb), dtype=torch.uint8, device="cuda", generator=g)
        ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        for _ in range(5):
            idx.search(q, k, out=(ids, dist))
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                idx.search(q, k, out=(ids, dist))
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            emit({"what": f"binary index search nq={nq} QPS", "value": round(nq / (ms * 1e-3), 1)})
    idx.free()
    seg.free()
    fseg = mq.VectorScanSegment.generate(0x5EED0001, 3, 1_000_000, 128, "L2", 8192)
    for _ in range(2):
        fidx = mq.VectorIndex.build(fseg, "MSTG", "nlist=1024")
        emit({"what": "float build_ms", "n": 1_000_000, "value": round(fidx.info()["build_ms"], 2)})
        fidx.free()
    fseg.free()


def reduce(path):
    rows = [json.loads(x) for x in open(path) if x.strip()]
    print("| figure | parent (min..max, median) | branch (min..max, median) | branch median inside |")
    print("|---|---|---|---|")
    for what in sorted({r["what"] for r in rows}):
        p = [r["value"] for r in rows if r["what"] == what and r["tag"] == "parent"]
        b = [r["value"] for r in rows if r["what"] == what and r["tag"] == "branch"]
        bm = statistics.median(b)
        better = bm > max(p) if "QPS" in what else bm < min(p)
        ok = "yes" if min(p) <= bm <= max(p) else "better" if better else "WORSE"
        print(f"| {what} | {min(p)}..{max(p)}, {statistics.median(p)} | {min(b)}..{max(b)}, {bm} | {ok} |")


if __name__ == "__main__":
    if sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    else:
        measure(sys.argv[1], sys.argv[2])
