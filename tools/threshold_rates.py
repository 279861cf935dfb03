"""Rates of the EDR and LCSS cells and of DTW at dim 2 of k_seqdp (csrc/seqdp.hip) beside Frechet's -- the table of DESIGN.md 3.19.

  python tools/threshold_rates.py [--dim 2]   every row: 2000 series of points uniform in [0, 2]^dim (eps = 1.0: 56 % of the point
                                              pairs match at dim 2), all 1 999 000 pairs i < j in one launch, lengths 20..60 (the
                                              (8, 16) shape), 400..500 (the (8, 64) shape) and 450..550 (the widest shape);
                                              "frechet_pairs", "dtw_pairs", "edr_pairs" and "lcss_pairs" on the same series, each warmed
                                              up once, then five rounds of one launch each in turn, device events
                                              (Engine.last_kernel_ms), min .. max, and the ratio of the median times to Frechet's
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from elastic_rates import CLASSES, all_pairs, cells   # noqa: E402


def series(nx, lo, hi, dim):
    rng = np.random.default_rng(lo + dim)
    return [rng.uniform(0.0, 2.0, size=(int(L), dim)) for L in rng.integers(lo, hi + 1, size=nx)]


def metrics():
    from annchor_amd import distances

    return {"frechet": distances.frechet, "dtw": distances.dtw, "dtw_window16": distances.DTW(window=16), "edr": distances.EDR(1.0),
            "edr_normalized": distances.EDR(1.0, normalize=True), "lcss": distances.LCSS(1.0), "lcss_delta16": distances.LCSS(1.0, delta=16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    from annchor_amd import _native

    IJ = all_pairs(args.nx)
    rows = []
    for lo, hi in CLASSES:
        X = series(args.nx, lo, hi, args.dim)
        engines = {}
        for name, metric in metrics().items():   # every measure bound and warmed up, then the launches alternate between them
            engines[name] = _native.Engine(0)
            metric.bind(engines[name], X)
            engines[name].metric_pairs(IJ)
        ms = {name: [] for name in engines}
        for _ in range(args.launches):
            for name, eng in engines.items():
                eng.metric_pairs(IJ)
                ms[name].append(eng.last_kernel_ms())
        for eng in engines.values():
            eng.close()
        base = float(np.median(ms["frechet"]))
        for name, t in ms.items():
            med = float(np.median(t))
            r = dict(kernel=name, dim=args.dim, lengths=[lo, hi], ms=t, cells=cells(X, IJ), gcells_per_s=cells(X, IJ) / (med * 1e-3) / 1e9,
                     ratio_to_frechet=med / base, spread=(max(t) - min(t)) / med)
            rows.append(r)
            print("%-15s dim %d  lengths %3d..%3d  %9.2f .. %9.2f ms   %8.1f Gcell/s   %.2f x frechet's time"
                  % (name, args.dim, lo, hi, min(t), max(t), r["gcells_per_s"], r["ratio_to_frechet"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
