"""Per variant: kernel launches and kernel time of the timed calls, from the
rocprofv3 kernel traces (setup kernels -- the generator, segment preparation --
are listed by name and left out of the per-call figures)."""
import csv
import glob
import json
import sys

SETUP = ("k_generate", "k_row_norms", "k_normalize", "k_to_hi", "k_max_norm", "k_pack", "k_fill_rows", "Cijk", "at::",
         "k_to_bf16")
root = sys.argv[1]
out = {}
for v in ("a", "b", "c_dev"):
    files = glob.glob(f"{root}/trace_{v}/**/*kernel_trace.csv", recursive=True)
    names = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"].split("(")[0]
            n = n.split("<")[0].replace("void mqvs::", "")
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            c = names.setdefault(n, [0, 0.0])
            c[0] += 1
            c[1] += dur
    calls = 10 + (1 if v.startswith("c") else 0)  # warmup 1 + rounds 9 (+ the stats call)
    search = {n: c for n, c in names.items() if not any(s in n for s in SETUP)}
    out[v] = dict(calls=calls,
                  launches_per_call=sum(c[0] for c in search.values()) / calls,
                  kernel_us_per_call=sum(c[1] for c in search.values()) / calls,
                  kernels={n: dict(count=c[0], us_per_call=round(c[1] / calls, 2)) for n, c in sorted(search.items())},
                  setup={n: c[0] for n, c in sorted(names.items()) if n not in search})
print(json.dumps(out, indent=1))
