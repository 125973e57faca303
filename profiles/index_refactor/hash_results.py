"""The index cases of tests/golden/make_search_plans.py, one search each:
writes, per case, the SHA-256 of the returned ids and of the distances' bits.
Run on two libraries, the outputs are equal exactly when every case returned
the same bytes (the first-stage cases return the list scan's own values).

    python profiles/index_refactor/hash_results.py <out.txt>
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
        h = hashlib.sha256()
        h.update(np.ascontiguousarray(ids, np.int64).tobytes())
        h.update(np.ascontiguousarray(dist, np.float32).view(np.uint32).tobytes())
        lines.append(f"{h.hexdigest()}  {plans.case_id(c)}\n")
    parts.free()
    with open(dst, "w") as f:
        f.writelines(lines)
    print(f"wrote {len(lines)} hashes to {dst}")


if __name__ == "__main__":
    main(sys.argv[1])
