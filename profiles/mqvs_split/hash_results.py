"""One call of everything mqvs.hip held before it was split -- every segment
constructor, from_column four ways (whole and ragged arrays, checksums on and
off), filtered and unfiltered FLAT searches at nq 1 and nq 20, a binary
search, both knn_*_raw functions, mqvs_merge_shards with host and with device
pointers, an ASYNC search followed by mqvs_async_check -- writing the SHA-256
of every returned array (and of each segment's info and resident rows).  Run
on two libraries under a kernel trace, the outputs and the ordered launch
lists are equal exactly when both made the same calls and returned the same
bytes.

    python profiles/mqvs_split/hash_results.py <out.txt>
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if hasattr(a, "cpu"):
            a = a.cpu().numpy()
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main(dst):
    import torch
    import myscaledb_amd as mq
    from myscaledb_amd import vector_scan as vs
    from oracle import oracle as O
    mq.init(0)
    lines = []

    def put(tag, *arrays):
        lines.append(f"{sha(*arrays)}  {tag}\n")

    def rows_of(seg):
        out = torch.empty((seg.n, seg.d), dtype=torch.float32, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")  # (device to device, into torch's memory)
        torch.cuda.synchronize()
        assert hip.hipMemcpy(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(seg.device_rows_ptr()),
                             ctypes.c_size_t(out.numel() * 4), 3) == 0
        return out

    def segment(tag, seg, q, k=10):
        info = seg.info()
        put(f"{tag}-info {sorted(info.items())}", repr(sorted(info.items())).encode())
        put(f"{tag}-rows", rows_of(seg))
        ids, dist = seg.search(q, k)
        put(f"{tag}-search", ids, dist.view(np.uint32))
        seg.free()

    # the constructors, on a part of 3 granules with empty arrays
    n, d, gran = 20000, 65, 8192
    rng = np.random.default_rng(7)
    rows = O.generate(0x5EED0001, 1, 0, n, d)
    q3 = O.generate(0x5EED0002, 1, 0, 3, d)
    ne = (rng.random(n) < 0.9).astype(np.uint8)
    ne[gran:2 * gran] = 0
    for metric in ("L2", "Cosine"):
        segment(f"create-{metric}", mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran), q3)
        segment(f"create-nonempty-{metric}",
                mq.VectorScanSegment.from_rows(rows, metric=metric, granule=gran, nonempty=ne), q3)
        segment(f"create_device-{metric}",
                mq.VectorScanSegment.from_rows(torch.from_numpy(rows).cuda(), metric=metric, granule=gran,
                                               nonempty=torch.from_numpy(ne).cuda()), q3)
        segment(f"generate-{metric}", mq.VectorScanSegment.generate(0x5EED0003, 2, n, d, metric=metric, granule=gran,
                                                                    row_offset=gran), q3)
    sizes_whole = np.full(n, d, np.uint64)
    sizes_ragged = rng.choice([0, d, d, d, d - 5, d + 7], n).astype(np.uint64)
    for shape, sizes in (("direct", sizes_whole), ("ragged", sizes_ragged)):
        data = rng.standard_normal(int(sizes.sum())).astype(np.float32)
        db = O.compress_stream(data.tobytes(), 1 << 18, 0x82)
        sb = O.compress_stream(sizes.tobytes(), 1 << 18, 0x82)
        for verify in (True, False):
            segment(f"from_column-{shape}-checksum={verify}",
                    mq.VectorScanSegment.from_column(db, sb, n, d, metric="Cosine", granule=gran,
                                                     verify_checksum=verify), q3)
    tdb = torch.frombuffer(bytearray(db), dtype=torch.uint8).cuda()
    tsb = torch.frombuffer(bytearray(sb), dtype=torch.uint8).cuda()
    segment("from_column-ragged-device", mq.VectorScanSegment.from_column(tdb, tsb, n, d, metric="L2", granule=gran),
            q3)

    # FLAT searches: filtered and not, nq 1 and nq 20 (the VALU and the batch paths)
    n, d = 300000, 96
    seg = mq.VectorScanSegment.generate(0x5EED0001, 2, n, d, metric="Cosine", granule=gran)
    flt = np.packbits(rng.random(n) < 0.3, bitorder="little")
    for nq in (1, 20):
        q = O.generate(0x5EED0004, 2, 0, nq, d)
        for tag, f in (("all", None), ("filtered", flt)):
            ids, dist = seg.search(q, 100, filter_bitmap=f)
            put(f"search-nq{nq}-{tag}", ids, dist.view(np.uint32))
    # an ASYNC search, then mqvs_async_check
    qd = torch.from_numpy(O.generate(0x5EED0004, 2, 0, 20, d)).cuda()
    ids, dist = seg.search(qd, 100, async_=True)
    vs.async_check()
    put("search-async", ids, dist.view(torch.int32))
    seg.free()

    # binary: segment, search, knn
    codes = rng.integers(0, 256, (50000, 17), dtype=np.uint8)
    qb = rng.integers(0, 256, (5, 17), dtype=np.uint8)
    for metric in ("Hamming", "Jaccard"):
        bseg = mq.BinaryVectorScanSegment.from_codes(codes, metric=metric, granule=gran)
        ids, dist = bseg.search(qb, 50)
        put(f"binary-search-{metric}", ids, dist.view(np.uint32))
        bseg.free()
        ids, dist = mq.try_brute_force_search_binary(qb, codes[:5000], 136, 20, 5, 5000, metric)
        put(f"knn_binary_raw-{metric}", ids, dist.view(np.uint32))
    for metric in ("L2", "IP"):
        ids, dist = mq.try_brute_force_search(q3, rows, 65, 20, 3, 20000, metric)
        put(f"knn_raw-{metric}", ids, dist.view(np.uint32))

    # merge: host and device pointers
    sh_ids = rng.integers(0, 1 << 40, (4, 6, 50)).astype(np.int64)
    sh_dist = np.sort(rng.random((4, 6, 50)).astype(np.float32), axis=2)
    oi, od = mq.merge_shards(sh_ids, sh_dist, "L2")
    put("merge-host", oi, od.view(np.uint32))
    oi, od = mq.merge_shards(torch.from_numpy(sh_ids).cuda(), torch.from_numpy(sh_dist).cuda(), "L2")
    put("merge-device", oi, od.view(torch.int32))

    with open(dst, "w") as f:
        f.writelines(lines)
    print(f"wrote {len(lines)} hashes to {dst}")


if __name__ == "__main__":
    main(sys.argv[1])
