"""Host planning of the searches, pinned: writes tests/golden/search_plans.json.

Every case is one search whose host-side plan (kernel path, gather decision,
probe length, segment count, rows scanned, re-scans) is read back from the
stats.  tests/test_gpu_plans.py replays the cases and compares those fields for
equality, so a change of the host pipeline that moves a plan shows up even when
the results stay bit-identical.  Times and the survivor / candidate counters
are not part of a plan.

    python tests/golden/make_search_plans.py <commit hash of the library>

The parts are generated on the device (mqvs_segment_generate); the float part
of 150000 x 64 rows is the smallest that gives a probe shorter than the part
and at least two main segments in every seg_tune class (kMinSegRows = 65536).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "search_plans.json")

N, N_SMALL, D, K = 150000, 3001, 64, 100
BIN_BITS = 256
SEARCH_FIELDS = ("path", "prefilter", "batch_kernel", "gather", "segments", "probe_rows", "main_rows",
                 "rows_scanned", "rescans", "nq", "k")
INDEX_FIELDS = ("nprobe", "num_reorder", "values", "items", "pairs", "plane_bytes", "pick_overflow", "reranked")
METRICS = ("L2", "IP", "Cosine")


def granule(metric):
    return 2048 if metric == "Cosine" else 8192


def cases():
    """The case list: dicts of plain values (the JSON names them by case_id)."""
    out = []
    for metric in METRICS:
        for nq in (1, 4, 19, 24, 200):
            for sel in (None, 0.05, 0.80):
                for exact in (False, True):
                    out.append(dict(kind="float", part="main", metric=metric, nq=nq, k=K, sel=sel, exact=exact))
    for metric in METRICS:
        # large k: query sub-batches under a 4 MiB scratch budget
        out.append(dict(kind="float", part="main", metric=metric, nq=8, k=5000, sel=None, exact=False,
                        scratch_budget=4 << 20))
        # the probe covers every row
        for nq in (1, 24, 200):
            out.append(dict(kind="float", part="small", metric=metric, nq=nq, k=K, sel=None, exact=False))
    for nq in (1, 50):
        out.append(dict(kind="binary", metric="Hamming", nq=nq, k=K))
    return out


def index_cases():
    """The two default builds, then float indexes of the main part built with an
    explicit nlist (`build`: a deterministic build, shared by the cases that
    name it), one case per branch of the index search's host code."""
    def ix(build, nq, params, metric="L2", k=K, **kw):
        return dict(kind="index", metric=metric, nq=nq, k=k, params=params, build=build, **kw)

    def bx(nq, params, metric="Hamming", k=K, **kw):
        return dict(kind="binary_index", metric=metric, nq=nq, k=k, params=params, build="nlist=64", **kw)

    return [dict(kind="index", metric="L2", nq=8, k=K, params="nprobe=8"),
            dict(kind="binary_index", metric="Hamming", nq=8, k=K, params="nprobe=8"),
            # pair mode (16 nq nprobe <= nlist), then the grouped plan with
            # 16-, 32- (24 nlist <= nq nprobe < 40 nlist) and 64-query items
            ix("nlist=4096", 8, "nprobe=8"),
            ix("nlist=64", 8, "nprobe=8"),
            ix("nlist=64", 200, "nprobe=8"),
            ix("nlist=64", 200, "nprobe=16"),
            # the coarse forms: every list probed (no ranking); nprobe above
            # kCoarsePickMaxT: the centroid list pass, and above kCoarseFlatLists
            # lists the FLAT search of the centroids (the pick: the cases above)
            ix("nlist=64", 8, "nprobe=64"),
            ix("nlist=256", 8, "nprobe=100"),
            ix("nlist=20000,kmeans_iters=2", 8, "nprobe=100"),
            # first stage only (the scan's own values), grouped and pair mode
            ix("nlist=64", 8, "nprobe=8", first_stage=True),
            ix("nlist=4096", 8, "nprobe=8", first_stage=True),
            # num_reorder = k: nothing to prune; every candidate re-ranked
            ix("nlist=64", 8, "nprobe=8,num_reorder=100"),
            ix("nlist=64", 8, "nprobe=8", rerank_all=True),
            ix("nlist=64", 8, "nprobe=8", sel=0.05),
            # cosine: the variant chain forks to the side stream (several chunk
            # ordinals: granule(metric)); under a filter the ordinals are recomputed
            ix("nlist=64", 8, "nprobe=8", metric="Cosine"),
            ix("nlist=64", 8, "nprobe=8", metric="Cosine", sel=0.05),
            ix("nlist=64", 8, "nprobe=8", metric="IP"),
            # fp8 list plane: pair mode, grouped, first stage of both, and the
            # centroid list pass (which rounds the queries to bf16 after all)
            ix("nlist=4096,plane=fp8", 8, "nprobe=8"),
            ix("nlist=64,plane=fp8", 8, "nprobe=8"),
            ix("nlist=4096,plane=fp8", 8, "nprobe=8", first_stage=True),
            ix("nlist=64,plane=fp8", 8, "nprobe=8", first_stage=True),
            ix("nlist=256,plane=fp8", 8, "nprobe=100"),
            # large k (num_reorder above kSortCap): query sub-batches under a 4 MiB scratch budget
            ix("nlist=64", 20, "nprobe=8", k=5000, scratch_budget=4 << 20),
            # binary index of the binary part (a Hamming part: Jaccard is the
            # search's metric): ranked probes, every list (no ranking), a
            # filter, k above kSortCap (the large select scratch), and query
            # sub-batches under a 1 MiB scratch budget
            bx(8, "nprobe=8"),
            bx(8, "nprobe=8,metric=Jaccard", metric="Jaccard"),
            bx(8, "nprobe=64"),
            bx(8, "nprobe=8", sel=0.05),
            bx(8, "nprobe=8", k=5000),
            bx(20, "nprobe=8", scratch_budget=1 << 20)]


def case_id(c):
    parts = [c["kind"], c.get("part", ""), c["metric"], f"nq{c['nq']}", f"k{c['k']}"]
    if c.get("sel") is not None:
        parts.append(f"sel{int(c['sel'] * 100)}")
    if c.get("exact"):
        parts.append("exact")
    if c.get("build"):
        # (index cases that name their build: the build, the search parameters and the flags)
        parts += [c["build"], c["params"]] + [f for f in ("first_stage", "rerank_all") if c.get(f)]
    return "-".join(p for p in parts if p)


def selection(n, frac):
    """A fixed scattered selection of about frac of n rows, as a bitmap."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    from myscaledb_amd import pack_bitmap
    return pack_bitmap(h < np.uint64(int(frac * 2 ** 32)))


class Parts:
    """The generated parts and indexes, built on first use and shared by the cases."""

    def __init__(self, mq):
        self.mq = mq
        self._segs = {}
        self._idx = {}

    def float_seg(self, part, metric):
        key = (part, metric)
        if key not in self._segs:
            n = N if part == "main" else N_SMALL
            self._segs[key] = self.mq.VectorScanSegment.generate(0x5EED0001, 1, n, D, metric=metric,
                                                                 granule=granule(metric))
        return self._segs[key]

    def binary_seg(self):
        if "bin" not in self._segs:
            rng = np.random.RandomState(0x5EED)
            codes = rng.randint(0, 256, size=(N, BIN_BITS // 8)).astype(np.uint8)
            self._segs["bin"] = self.mq.BinaryVectorScanSegment.from_codes(codes, metric="Hamming")
        return self._segs["bin"]

    def index(self, kind, metric="L2", build=None):
        # (a binary index is the Hamming part's whatever metric its search names)
        key = (kind, metric if kind == "index" else "Hamming", build)
        if key not in self._idx:
            if kind == "index":
                self._idx[key] = self.mq.VectorIndex.build(self.float_seg("main", metric), "MSTG", build)
            else:
                self._idx[key] = self.mq.BinaryVectorIndex.build(self.binary_seg(), "BINARYMSTG", build)
        return self._idx[key]

    def free(self):
        for x in list(self._idx.values()) + list(self._segs.values()):
            x.free()
        self._idx, self._segs = {}, {}


def float_queries(nq):
    from oracle import oracle as O
    return O.generate(0x5EED0002, 1, 0, nq, D)


def binary_queries(nq):
    return np.random.RandomState(0xB17 + nq).randint(0, 256, size=(nq, BIN_BITS // 8)).astype(np.uint8)


def search_index_case(parts, c):
    """The search of one index case; returns (ids, dist) as host arrays."""
    from myscaledb_amd import vector_scan
    idx = parts.index(c["kind"], c["metric"], c.get("build"))
    flt = None if c.get("sel") is None else selection(idx.segment.n, c["sel"])
    prev = vector_scan.set_scratch_budget(c["scratch_budget"]) if c.get("scratch_budget") else None
    try:
        if c["kind"] == "binary_index":
            return idx.search(binary_queries(c["nq"]), c["k"], c["params"], filter_bitmap=flt)
        return idx.search(float_queries(c["nq"]), c["k"], c["params"], filter_bitmap=flt,
                          first_stage_only=bool(c.get("first_stage")), rerank_all=bool(c.get("rerank_all")))
    finally:
        if prev is not None:
            vector_scan.set_scratch_budget(prev)


def run_case(parts, c):
    """One search; returns the plan fields of its stats."""
    from myscaledb_amd import _lib, vector_scan
    if c["kind"] == "float":
        seg = parts.float_seg(c["part"], c["metric"])
        flt = None if c.get("sel") is None else selection(seg.n, c["sel"])
        prev = vector_scan.set_scratch_budget(c["scratch_budget"]) if c.get("scratch_budget") else None
        try:
            seg.search(float_queries(c["nq"]), c["k"], filter_bitmap=flt, exact=bool(c.get("exact")))
        finally:
            if prev is not None:
                vector_scan.set_scratch_budget(prev)
        st = _lib.last_search_stats()
        return {f: int(st[f]) for f in SEARCH_FIELDS}
    if c["kind"] == "binary":
        parts.binary_seg().search(binary_queries(c["nq"]), c["k"])
        st = _lib.last_search_stats()
        return {f: int(st[f]) for f in SEARCH_FIELDS}
    search_index_case(parts, c)
    st = _lib.last_index_stats()
    return {f: int(st[f]) for f in INDEX_FIELDS}


def write(doc, path):
    """One case per line: its id (case_id: the case itself is in cases() / index_cases()) and its plan."""
    rows = ",\n".join(' %s: %s' % (json.dumps(e["id"]), json.dumps(e["plan"], sort_keys=True)) for e in doc["cases"])
    with open(path, "w") as f:
        f.write('{"library_commit": %s, "plans": {\n%s\n}}\n' % (json.dumps(doc["library_commit"]), rows))


def main():
    import myscaledb_amd as mq
    mq.init(0)
    with_index = "--no-index" not in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parts = Parts(mq)
    todo = cases() + (index_cases() if with_index else [])
    doc = {"library_commit": args[0] if args else "unknown", "cases": []}
    for c in todo:
        doc["cases"].append({"id": case_id(c), "case": c, "plan": run_case(parts, c)})
    parts.free()
    out = args[1] if len(args) > 1 else OUT
    write(doc, out)
    print(f"wrote {len(doc['cases'])} plans to {out}")


if __name__ == "__main__":
    main()
