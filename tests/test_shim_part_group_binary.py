"""The binary part-group part of the reference-side C++ binding
(include/mqvs_vector_index.hpp: BinaryPartGroup over BinaryPartScans) compiled
with g++ against libmqvs.so.  CPU: the calls' status -> DB::Exception mappings.
GPU: BinaryPartGroup::search returns the oracle's labelled rows
(O.vector_scan_binary per part, O.merge_parts per query, padding dropped) for a
Hamming and a Jaccard case with a filter."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAN = 256


@pytest.fixture(scope="module")
def shim_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim_part_group_binary") / "shim_part_group_binary"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DMQVS_SHIM_STANDALONE",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/shim/shim_part_group_binary.cpp"),
           "-L", os.path.join(ROOT, "myscaledb_amd"), "-l:libmqvs.so",
           "-Wl,-rpath," + os.path.join(ROOT, "myscaledb_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_shim_part_group_binary_maps_errors(shim_bin):
    r = subprocess.run([shim_bin, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "errors ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_shim_part_group_binary_gpu(shim_bin, tmp_path, metric):
    rng = np.random.default_rng(12000)
    nbytes, nq, k = 4, 3, 60
    sizes, offsets = (700, 257, 30), (0, 3 * GRAN, 8 * GRAN)
    parts = [np.packbits(rng.random((n, nbytes * 8)) < 0.5, axis=1) for n in sizes]
    queries = np.packbits(rng.random((nq, nbytes * 8)) < 0.5, axis=1)
    bits = lambda mask: np.packbits(mask.astype(np.uint8), bitorder="little")
    filters = [bits(rng.random(sizes[0]) < 0.05), None, None]  # 35 rows or so: k passes parts 0 and 2
    exists = [None, bits(rng.random(sizes[1]) >= 0.3), None]
    m = O.METRICS[metric]

    # the oracle's labelled rows: query-major, best first, padding dropped
    lists = []
    for p, codes in enumerate(parts):
        ids, dist = O.vector_scan_binary(codes, queries, k, m, GRAN, filter_bits=filters[p], row_exists_bits=exists[p])
        lists.append((np.where(ids >= 0, ids + offsets[p], ids), dist))
    want = []
    for q in range(nq):
        part, ids, dist = O.merge_parts(np.stack([l[0][q] for l in lists]), np.stack([l[1][q] for l in lists]), m)
        want += [(int(part[i]), int(ids[i]), q, dist[i].tobytes()) for i in range(k) if ids[i] >= 0]
    assert len({w[0] for w in want}) == 3, "inputs lost a part from the result"

    blob = struct.pack("<5i", len(parts), nbytes, nq, k, m)
    for p, codes in enumerate(parts):
        blob += struct.pack("<2q", sizes[p], offsets[p]) + codes.tobytes()
        for bm in (filters[p], exists[p]):
            blob += b"\0" if bm is None else b"\1" + bm.tobytes()
    blob += queries.tobytes()
    src, dst = tmp_path / "case.bin", tmp_path / "rows.bin"
    src.write_bytes(blob)

    r = subprocess.run([shim_bin, "gpu", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("fused 1", "bad width 1", "fallback 1"):
        assert tag in r.stdout, r.stdout
    out = dst.read_bytes()
    (rows,) = struct.unpack_from("<q", out)
    rec = np.frombuffer(out, np.dtype([("part", "<u4"), ("label", "<u4"), ("vector_id", "<u4"), ("dist", "V4")]),
                        count=rows, offset=8)
    got = [(int(r_["part"]), int(r_["label"]), int(r_["vector_id"]), r_["dist"].tobytes()) for r_ in rec]
    assert got == want
