"""rocprofv3 --kernel-trace CSV -> a short summary of the dispatches:

* line 1: the number of dispatches and the SHA-256 of the ordered list
  "kernel name <tab> grid <tab> workgroup", one line per dispatch in dispatch
  order -- two runs queued the same launches in the same order exactly when
  these lines are equal;
* then the dispatch count per kernel name, to see what a difference is about.

    python reduce_trace.py <..._kernel_trace.csv> <out.txt>
"""
import collections
import csv
import hashlib
import sys


def main(src, dst):
    with open(src, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    h = hashlib.sha256()
    names = collections.Counter()
    for r in rows:
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        h.update(f"{r['Kernel_Name']}\t{grid}\t{wg}\n".encode())
        names[r["Kernel_Name"]] += 1
    with open(dst, "w") as f:
        f.write(f"{len(rows)} dispatches, ordered (kernel, grid, workgroup) sha256 {h.hexdigest()}\n")
        for name, n in sorted(names.items()):
            f.write(f"{n}\t{name}\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
