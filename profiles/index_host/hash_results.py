"""Every index case of tests/golden/make_search_plans.py (float and binary),
one search each, then one float and one binary build: writes, per case, the
SHA-256 of the returned ids and of the distances' bits, and per build the
SHA-256 of lists(), of centroids() and of the saved blob.  Run on two
libraries, the outputs are equal exactly when every case returned the same
bytes and the builds made the same index.  The two blobs are also written
beside the output (<out>.float.blob, <out>.binary.blob) for a byte compare.

    python profiles/index_host/hash_results.py <out.txt>
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main(dst):
    spec = importlib.util.spec_from_file_location(
        "make_search_plans", os.path.join(ROOT, "tests", "golden", "make_search_plans.py"))
    plans = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plans)
    import myscaledb_amd as mq
    mq.init(0)
    parts = plans.Parts(mq)
    lines = []
    for c in plans.index_cases():
        ids, dist = plans.search_index_case(parts, c)
        lines.append(f"{sha(np.asarray(ids, np.int64), np.asarray(dist, np.float32).view(np.uint32))}  "
                     f"{plans.case_id(c)}\n")
    for kind, tag in (("index", "float"), ("binary_index", "binary")):
        # (a build of its own, not the cases' shared one)
        seg = parts.float_seg("main", "L2") if kind == "index" else parts.binary_seg()
        cls = mq.VectorIndex if kind == "index" else mq.BinaryVectorIndex
        idx = cls.build(seg, "MSTG" if kind == "index" else "BINARYMSTG", "nlist=96")
        blob = idx.save()
        lines.append(f"{sha(*idx.lists())}  build-{tag}-nlist=96-lists\n")
        lines.append(f"{sha(idx.centroids())}  build-{tag}-nlist=96-centroids\n")
        lines.append(f"{sha(blob)}  build-{tag}-nlist=96-blob ({len(blob)} bytes)\n")
        with open(f"{dst}.{tag}.blob", "wb") as f:
            f.write(blob)
        idx.free()
    parts.free()
    with open(dst, "w") as f:
        f.writelines(lines)
    print(f"wrote {len(lines)} hashes to {dst}")


if __name__ == "__main__":
    main(sys.argv[1])
