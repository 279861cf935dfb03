"""Aggregate rocprofv3 PMC passes into profiles/rNN_pmc_traffic.json.

    python tools/pmc_summary.py <fetch_dir> <write_dir> <out.json>

<fetch_dir> / <write_dir> are the -d directories of two separate runs of the same command,
    rocprofv3 --pmc FETCH_SIZE  --output-format csv -d <fetch_dir> -o pmc -- python bench.py --full ...
    rocprofv3 --pmc WRITE_SIZE  --output-format csv -d <write_dir> -o pmc -- python bench.py --full ...
(never combined with a trace domain).  Units: KiB per dispatch.  Correction as prescribed by
MI355X_MICROARCH.md (HBM section): FETCH_SIZE is doubled on gfx950; WRITE_SIZE is taken as is.
hbm_bytes_per_launch_corrected = (2 * FETCH + WRITE) * 1024 / launches."""
import csv, glob, json, os, sys
from collections import defaultdict


def collect(d, counter):
    agg = defaultdict(lambda: [0, 0.0])
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") != counter:
                continue
            name = row["Kernel_Name"].replace("void ", "").split("(")[0]
            a = agg[name]
            a[0] += 1
            a[1] += float(row["Counter_Value"])
    return agg


def main():
    fetch, write, out = sys.argv[1:4]
    F, W = collect(fetch, "FETCH_SIZE"), collect(write, "WRITE_SIZE")
    res = {}
    for name in sorted(set(F) | set(W)):
        n = max(F.get(name, [0])[0], W.get(name, [0])[0])
        f, w = F.get(name, [0, 0.0])[1], W.get(name, [0, 0.0])[1]
        res[name] = {"launches": n, "fetch_KiB_raw": round(f / max(n, 1), 1), "write_KiB_raw": round(w / max(n, 1), 1),
                     "hbm_bytes_per_launch_corrected": int((2 * f + w) * 1024 / max(n, 1))}
    json.dump(res, open(out, "w"), indent=1)
    print("wrote", out, len(res), "kernels")


if __name__ == "__main__":
    main()
