"""Rates of k_hauswide (csrc/hauswide.hip: Hausdorff at 5 .. 512 coordinates per point) beside the yardstick, k_hausdorff at dim 4
(csrc/hausdorff.hip), on the same three length ranges -- the table of DESIGN.md 3.11a.

  python tools/hauswide_rates.py          random sets, all pairs i < j of 128 members in one launch: 20..60, 400..500 and 3000..4000
                                          points; dims 5, 16, 64, 384 and, on k_hausdorff, 4; float32 and float64; both tile shapes
                                          (ANNCHOR_HAUSW_SHAPE = 32, 64: every data set can take either) and the one the launch
                                          picks; one warm-up, then five launches, device events (Engine.last_kernel_ms), median
                                          and min .. max.  A figure is ps per cell-coordinate, ms / (n m dim) summed over the
                                          pairs -- k_hausdorff evaluates each of those cells twice, k_hauswide once; `share` is
                                          3 n m dim float64 operations over the time, against 39.3e12 / s (one float64
                                          instruction per lane and clock: DESIGN.md 3.11).
  python tools/hauswide_rates.py --cross  where the two shapes cross: 512 members of 1 .. L points for L = 48 .. 512, dims 16 and
                                          64, float64, both shapes forced
  python tools/hauswide_rates.py --fit    the fit of tests/test_hauswide_gpu.py (120 clustered sets of 20 .. 60 points, dim 16),
                                          device metric against hausdorff_pair_host as a Python metric on the host
  python tools/hauswide_rates.py --one DIM LO HI [--dtype float32] [--shape 32]
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

ROWS = ((20, 60), (400, 500), (3000, 4000))
DIMS = (5, 16, 64, 384)
PEAK = 39.3e12   # float64 instructions per second, one per lane and clock


def sets(nx, lo, hi, dim, dtype):
    rng = np.random.default_rng(lo + dim)
    return [rng.standard_normal((int(L), dim)).astype(dtype) for L in rng.integers(lo, hi + 1, size=nx)]


def row(nx, lo, hi, dim, dtype, launches, shape=None):
    from annchor_amd import distances

    if shape:
        os.environ["ANNCHOR_HAUSW_SHAPE"] = str(shape)   # (read per launch)
    else:
        os.environ.pop("ANNCHOR_HAUSW_SHAPE", None)
    X, IJ = sets(nx, lo, hi, dim, dtype), all_pairs(nx)
    n = cells(X, IJ)
    ms = timed(distances.Hausdorff(wide=True), X, IJ, launches)
    med = float(np.median(ms))
    r = dict(dim=dim, dtype=np.dtype(dtype).name, nx=nx, lengths=[lo, hi], shape=shape, ms=ms, cells=n, us_per_pair=med * 1e3 / len(IJ),
             ps_per_cell_coord=med * 1e9 / (n * dim), share=3.0 * n * dim / (med * 1e-3) / PEAK)
    print("dim %3d %-7s %4d of %4d..%4d  shape %-4s median %9.3f ms (%9.3f .. %9.3f)  %8.3f us/pair  %7.3f ps/cell-coord  %5.1f %% of float64 issue"
          % (dim, r["dtype"], nx, lo, hi, shape or "auto", med, min(ms), max(ms), r["us_per_pair"], r["ps_per_cell_coord"], 100 * r["share"]),
          flush=True)
    return r


def table(nx, launches):
    out = []
    for lo, hi in ROWS:
        for dtype in (np.float32, np.float64):
            out.append(row(nx, lo, hi, 4, dtype, launches))   # k_hausdorff: the yardstick (its share counts its cells once, too)
            for dim in DIMS:
                few = dim * hi > 1 << 19   # (128 sets of 3000 .. 4000 points at dim 384 are 1.4 GB in float64 and 1.1e14 operations: half the sets)
                out += [row(nx // 2 if few else nx, lo, hi, dim, dtype, launches, shape) for shape in (32, 64)]
    return out


def cross(launches):
    return [row(512, 1, L, dim, np.float64, launches, shape) for dim in (16, 64) for L in (48, 64, 96, 128, 192, 256, 384, 512)
            for shape in (32, 64)]


def fits():
    from annchor_amd import Annchor

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import hausdorff_cases as hc
    import pool_cases as pc

    os.environ.pop("ANNCHOR_HAUSW_SHAPE", None)
    X = hc.clustered_curves(120, 20, 60, 16, seed=93)
    out = {}
    for label, metric, kw in (("device", "hausdorff", {"func_kwargs": {"wide": True}}), ("python", hc.hausdorff_pair_host, {})):
        secs = []
        for _ in range(3 if label == "device" else 1):
            t0 = time.perf_counter()
            ann = Annchor(X, metric, ols="lapack", **kw, **pc.FIT_CFG).fit()
            secs.append(time.perf_counter() - t0)
        out[label] = dict(seconds=secs, evals=int(ann.evals))
        print("fit, %s metric: %s s, %d evaluations" % (label, ", ".join("%.4f" % s for s in secs), ann.evals), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, type=int, metavar=("DIM", "LO", "HI"))
    ap.add_argument("--cross", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--shape", type=int, default=None)
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    if args.one:
        out = dict(rows=[row(args.nx, args.one[1], args.one[2], args.one[0], np.dtype(args.dtype).type, 1, args.shape)])
    elif args.cross:
        out = dict(rows=cross(args.launches))
    elif args.fit:
        out = dict(fits=fits())
    else:
        out = dict(rows=table(args.nx, args.launches))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
