"""Rates of k_seqwide (csrc/seqwide.hip: DTW and Frechet at 5 .. 64 coordinates per point), k_editwide (csrc/editwide.hip: ERP
and TWE there) and k_threshwide (csrc/threshwide.hip: EDR and LCSS there) beside the yardstick, k_seqdp at dim 4 (csrc/seqdp.hip),
on the same three length ranges -- the tables of DESIGN.md 3.19a, 3.19b and 3.19c; an ERP, TWE, EDR or LCSS row also carries its
time over k_seqwide's Frechet on the same members and dtype.  EDR and LCSS run at two thresholds: eps 1.0, at which the walks'
points hardly ever match and a row's match word is 0 after its first chunk of coordinates, and eps 1e9, at which every pair of
points matches and no row ends early.

  python tools/seqwide_rates.py          random walks, all pairs i < j in one launch: 1500 members of 20..60 points, 256 of 400..500,
                                         128 of 900..1000; dims 5, 8, 13, 39, 64 and, on k_seqdp, 4; float32 and float64; one warm-up,
                                         then five launches, device events (Engine.last_kernel_ms), median and min .. max.  A figure
                                         is ns per cell-coordinate, ms / (cells x dim); `ratio` is that figure over 14/12 of k_seqdp's
                                         on the same lengths and dtype, what a kernel bound by float64 issue alone would reach.
                                         Then DTW at window = 8 against unbanded on the longest shape, and the dim-13 fit of the
                                         tests against the same fit with the recurrence as a Python metric on the host.
  python tools/seqwide_rates.py --one DIM LO HI [--metric NAME] [--dtype float32]
                                         one warm-up and one launch of one row: what a counter run wraps
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wed_rates import all_pairs, cells, timed   # noqa: E402  (adds the repository to sys.path)

ROWS = ((1500, 20, 60), (256, 400, 500), (128, 900, 1000))
MEASURES = (("dtw", {}), ("frechet", {}), ("erp", {}), ("twe", {}), ("edr", {"eps": 1.0}), ("edr", {"eps": 1e9}), ("lcss", {"eps": 1.0}),
            ("lcss", {"eps": 1e9}))
DIMS = (5, 8, 13, 39, 64)


def walks(nx, lo, hi, dim, dtype):
    rng = np.random.default_rng(lo + dim)
    return [np.cumsum(rng.standard_normal((int(L), dim)), axis=0).astype(dtype) for L in rng.integers(lo, hi + 1, size=nx)]


def row(name, kw, nx, lo, hi, dim, dtype, launches):
    from annchor_amd.utils import get_function_from_input

    X, IJ = walks(nx, lo, hi, dim, dtype), all_pairs(nx)
    n = cells(X, IJ)
    ms = timed(get_function_from_input(name, dict(kw, wide=True)), X, IJ, launches)
    r = dict(metric=name, kw=kw, dim=dim, dtype=np.dtype(dtype).name, nx=nx, lengths=[lo, hi], ms=ms, cells=n,
             gcells_per_s=n / (np.median(ms) * 1e-3) / 1e9, ns_per_cell_coord=np.median(ms) * 1e6 / (n * dim))
    print("%-8s %-12s dim %2d %-7s %4d of %3d..%4d  median %9.3f ms (%9.3f .. %9.3f)  %7.2f Gcell/s  %7.4f ns/cell-coord"
          % (name, kw or "", dim, r["dtype"], nx, lo, hi, np.median(ms), min(ms), max(ms), r["gcells_per_s"], r["ns_per_cell_coord"]), flush=True)
    return r


def table(launches, metrics):
    out = []
    for nx, lo, hi in ROWS:
        for dtype in (np.float32, np.float64):
            frechet = {}   # k_seqwide's Frechet on the same members: the yardstick of k_editwide's rows (it runs first)
            for name, kw in [m for m in MEASURES if m[0] in metrics]:
                base = row(name, kw, nx, lo, hi, 4, dtype, launches)   # k_seqdp: the yardstick
                out.append(base)
                for dim in DIMS:
                    r = row(name, kw, nx, lo, hi, dim, dtype, launches)
                    r["ratio"] = r["ns_per_cell_coord"] / (base["ns_per_cell_coord"] * 14.0 / 12.0)
                    print("    ratio to 14/12 of k_seqdp at dim 4: %.2f" % r["ratio"], flush=True)
                    if name == "frechet":
                        frechet[dim] = float(np.median(r["ms"]))
                    elif name in ("erp", "twe", "edr", "lcss") and dim in frechet:
                        r["over_frechet"] = float(np.median(r["ms"])) / frechet[dim]
                        print("    time over k_seqwide's Frechet on the same members: %.2f" % r["over_frechet"], flush=True)
                    out.append(r)
    nx, lo, hi = ROWS[-1]
    for dim in (13, 64) if "dtw" in metrics else ():
        for kw in ({}, {"window": 8}):
            out.append(row("dtw", kw, nx, lo, hi, dim, np.float64, launches))
    return out


def dtw_python(x, y):
    """The recurrence as a Python metric: c(i, j) a coordinate at a time, then the double loop."""
    t = x[:, None, 0] - y[None, :, 0]
    c = t * t
    for k in range(1, x.shape[1]):
        t = x[:, None, k] - y[None, :, k]
        c = c + t * t
    c = c.tolist()
    inf = float("inf")
    prev = [inf] * len(y)
    for i, ci in enumerate(c):
        cur, left = [], inf
        for j, v in enumerate(ci):
            dg = prev[j - 1] if j else (0.0 if i == 0 else inf)
            left = v + min(left, prev[j], dg)
            cur.append(left)
        prev = cur
    return prev[-1] ** 0.5


def erp_python(x, y):
    """ERP at gap 0 as a Python metric: dist a coordinate at a time, then the double loop."""
    def dist(a, b):
        t = a[..., 0] - b[..., 0]
        c = t * t
        for k in range(1, a.shape[-1]):
            t = a[..., k] - b[..., k]
            c = c + t * t
        return np.sqrt(c)

    c = dist(x[:, None, :], y[None, :, :]).tolist()
    gx, gy = dist(x, np.zeros_like(x)).tolist(), dist(y, np.zeros_like(y)).tolist()
    prev = [0.0]
    for g in gy:
        prev.append(prev[-1] + g)
    left = 0.0
    for ci, gxi in zip(c, gx):
        left = left + gxi
        cur = [left]
        for j, v in enumerate(ci):
            cur.append(min(prev[j] + v, prev[j + 1] + gxi, cur[j] + gy[j]))
        prev = cur
    return prev[-1]


def fits(metrics):
    """The fits of tests/test_seqwide_gpu.py and tests/test_editwide_gpu.py (160 clustered curves of 20 .. 60 points at dim 13),
    device metric and host metric."""
    from annchor_amd import Annchor

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import pool_cases as pc
    import seqdp_cases as sc

    X = sc.clustered_curves(160, 20, 60, 13, seed=93)
    out = {}
    for name, python, is_metric in (("dtw", dtw_python, False), ("erp", erp_python, True)):
        if name not in metrics:
            continue
        for label, metric, kw in (("device", name, {"func_kwargs": {"wide": True}}), ("python", python, {})):
            secs = []
            for _ in range(3 if label == "device" else 1):
                t0 = time.perf_counter()
                ann = Annchor(X, metric, is_metric=is_metric, ols="lapack", **kw, **pc.FIT_CFG).fit()
                secs.append(time.perf_counter() - t0)
            out[name + ", " + label] = dict(seconds=secs, evals=int(ann.evals))
            print("%s fit, %s metric: %s s, %d evaluations" % (name, label, ", ".join("%.3f" % s for s in secs), ann.evals), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, type=int, metavar=("DIM", "LO", "HI"))
    ap.add_argument("--metric", default="dtw", help="--one: dtw, frechet, erp, twe, edr or lcss")
    ap.add_argument("--eps", type=float, default=1.0, help="--one: the threshold of edr and lcss")
    ap.add_argument("--metrics", nargs="+", default=["dtw", "frechet", "erp", "twe", "edr", "lcss"], help="the table's measures")
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    if args.one:
        kw = {"eps": args.eps} if args.metric in ("edr", "lcss") else {}
        out = dict(rows=[row(args.metric, kw, args.nx, args.one[1], args.one[2], args.one[0], np.dtype(args.dtype).type, 1)])
    else:
        out = dict(rows=table(args.launches, args.metrics), fits=fits(args.metrics))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
