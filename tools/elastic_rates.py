"""Rates of the MSM and TWE cells of k_seqdp (csrc/seqdp.hip) beside ERP's -- the tables of DESIGN.md 3.16 and 3.17.

  python tools/elastic_rates.py               every row: 2000 random walks, all 1 999 000 pairs i < j in one launch, lengths 20..60
                                              (the (8, 16) shape), 400..500 (the (8, 64) shape) and 450..550 (the widest shape);
                                              "erp_pairs", "msm_pairs" and "twe_pairs" on the same series; one warm-up, then
                                              three launches, device events (Engine.last_kernel_ms), min .. max, and the ratio of
                                              the medians to ERP's
  python tools/elastic_rates.py --dim 2       the same with points of `dim` coordinates: ERP and TWE only
  python tools/elastic_rates.py --one twe 400 500    one warm-up and one launch of one row: what a counter run wraps
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CLASSES = ((20, 60), (400, 500), (450, 550))


def all_pairs(nx):
    i, j = np.triu_indices(nx, 1)
    return np.stack([i, j], axis=1).astype(np.int64)


def walks(nx, lo, hi, dim):
    rng = np.random.default_rng(lo + dim)
    X = [np.cumsum(rng.standard_normal((int(L), dim)), axis=0) for L in rng.integers(lo, hi + 1, size=nx)]
    return [x[:, 0] for x in X] if dim == 1 else X


def timed(metric, X, IJ, launches):
    from annchor_amd import _native

    eng = _native.Engine(0)
    metric.bind(eng, X)
    eng.metric_pairs(IJ)   # warm-up
    ms = []
    for _ in range(launches):
        eng.metric_pairs(IJ)
        ms.append(eng.last_kernel_ms())
    eng.close()
    return ms


def cells(X, IJ):
    L = np.array([len(x) for x in X], dtype=np.float64)
    return float((L[IJ[:, 0]] * L[IJ[:, 1]]).sum())


def metrics(dim):
    from annchor_amd import distances

    m = {"erp": distances.erp, "twe": distances.twe}
    if dim == 1:
        m["msm"] = distances.msm
    return m


def rates(nx, launches, dim):
    IJ = all_pairs(nx)
    rows = []
    for lo, hi in CLASSES:
        X = walks(nx, lo, hi, dim)
        erp_ms = None
        for name, metric in metrics(dim).items():
            ms = timed(metric, X, IJ, launches)
            if name == "erp":
                erp_ms = float(np.median(ms))
            r = dict(kernel=name + "_pairs", dim=dim, lengths=[lo, hi], ms=ms, cells=cells(X, IJ))
            r["gcells_per_s"] = r["cells"] / (np.median(ms) * 1e-3) / 1e9
            r["ratio_to_erp"] = float(np.median(ms)) / erp_ms
            rows.append(r)
            print("%-10s dim %d  lengths %3d..%3d  %9.2f .. %9.2f ms   %8.1f Gcell/s   %.2f x erp"
                  % (r["kernel"], dim, lo, hi, min(ms), max(ms), r["gcells_per_s"], r["ratio_to_erp"]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("METRIC", "LO", "HI"))
    ap.add_argument("--dim", type=int, default=1)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    if args.one:
        name, lo, hi = args.one[0], int(args.one[1]), int(args.one[2])
        ms = timed(metrics(args.dim)[name], walks(args.nx, lo, hi, args.dim), all_pairs(args.nx), 1)
        print("%s_pairs dim %d lengths %d..%d: %.2f ms" % (name, args.dim, lo, hi, ms[0]), flush=True)
        return
    out = rates(args.nx, args.launches, args.dim)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
