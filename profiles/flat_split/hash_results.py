"""One call of each shape the group searches of part_group.hip serve -- float
L2 and cosine at nq 1 and at nq 20 with the batch route opted in, binary
Hamming and Jaccard at nq 1 and nq 20, each with host and with device
pointers, with and without bitmaps, over a group one of whose parts is above
the row limit -- writing the SHA-256 of every returned array and the call's
stats.  Run on two libraries under a kernel trace, the outputs and the ordered
launch lists are equal exactly when both made the same calls and returned the
same bytes.

    python profiles/flat_split/hash_results.py <out.txt>
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (5, 300, 700, 4000)  # the last one above the row limit set below
LIMIT = 2048


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if hasattr(a, "cpu"):
            a = a.cpu().numpy()
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main(dst):
    import torch
    import myscaledb_amd as mq
    from oracle import oracle as O
    mq.init(0)
    lines = []
    rng = np.random.default_rng(11)
    masks = [[np.packbits(rng.random(n) < p, bitorder="little") for n in SIZES] for p in (0.4, 0.9)]
    masks[0][1] = None  # (a part without a filter among filtered ones)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()

    def run(tag, group, queries, k, metric):
        for where, q, bm in (("host", queries, masks), ("device", dev(queries), [[dev(m) for m in ms] for ms in masks])):
            for name, f, e in (("plain", None, None), ("bitmaps", bm[0], bm[1])):
                torch.cuda.synchronize()
                part, ids, dist = group.search(q, k, metric=metric, filters=f, row_exists=e)
                st = group.last_stats()
                if where == "device":
                    dist = dist.view(torch.int32)
                else:
                    dist = dist.view(np.uint32)
                lines.append(f"{sha(part, ids, dist)}  {tag}-{where}-{name} {sorted(st.items())}\n")

    prev = mq.set_part_group_rows(LIMIT), mq.set_part_group_binary_rows(LIMIT), mq.part_group_batch()
    mq.set_part_group_batch(LIMIT)
    try:
        for metric in ("L2", "Cosine"):
            segs = [mq.VectorScanSegment.from_rows(O.generate(0x5EED0100 + p, 1, 0, n, 24), metric=metric, granule=256)
                    for p, n in enumerate(SIZES)]
            group = mq.PartGroup(segs)
            for nq in (1, 20):
                run(f"float-{metric}-nq{nq}", group, O.generate(0x5EED0200, 1, 0, nq, 24), 10, metric)
            group.free()
            for s in segs:
                s.free()
        codes = [rng.integers(0, 256, (n, 8), dtype=np.uint8) for n in SIZES]
        segs = [mq.BinaryVectorScanSegment.from_codes(c, granule=256) for c in codes]
        group = mq.BinaryPartGroup(segs)
        for metric in ("Hamming", "Jaccard"):
            for nq in (1, 20):
                run(f"binary-{metric}-nq{nq}", group, rng.integers(0, 256, (nq, 8), dtype=np.uint8), 10, metric)
        group.free()
        for s in segs:
            s.free()
    finally:
        mq.set_part_group_rows(prev[0])
        mq.set_part_group_binary_rows(prev[1])
        mq.set_part_group_batch(*prev[2])

    with open(dst, "w") as f:
        f.writelines(lines)
    print(f"wrote {len(lines)} hashes to {dst}")


if __name__ == "__main__":
    main(sys.argv[1])
