"""Rates of the indel (LCS) kernels (csrc/indel.hip, k_indel_f) beside "levenshtein"'s (csrc/lev.hip, k_lev_f / k_lev_r<1>) on the
same strings and the same pair lists -- the table of DESIGN.md 3.15d.

  python tools/indel_rates.py         random strings over 26 symbols, all pairs i < j in one launch -- 2000 strings of 20..60 and of
                                      400..500 symbols, 1000 strings of 900..1000 (all k_indel_f<1>) and 1000 of 1500..2000
                                      (k_indel_f<2>; "levenshtein": k_lev_r<1>); one warm-up, then five launches, device events
                                      (Engine.last_kernel_ms), median and min .. max
  python tools/indel_rates.py --one LO HI [--metric NAME]
                                      one warm-up and one launch of one row: what a counter run wraps
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wed_rates import all_pairs, cells, strings, timed   # noqa: E402  (adds the repository to sys.path)

A = 26
ROWS = ((2000, 20, 60), (2000, 400, 500), (1000, 900, 1000), (1000, 1500, 2000))


def rates(rows, names, launches):
    from annchor_amd.utils import get_function_from_input

    out = []
    for nx, lo, hi in rows:
        IJ = all_pairs(nx)
        X = strings(nx, lo, hi, A, seed=A + lo)
        n = cells(X, IJ)
        for name in names:
            ms = timed(get_function_from_input(name, None), X, IJ, launches)
            out.append(dict(kernel=name, nx=nx, lengths=[lo, hi], A=A, ms=ms, cells=n, gcells_per_s=n / (np.median(ms) * 1e-3) / 1e9))
            print("%-12s %4d strings of %4d..%4d  median %9.3f ms  (%9.3f .. %9.3f)   %9.1f Gcell/s"
                  % (name, nx, lo, hi, np.median(ms), min(ms), max(ms), out[-1]["gcells_per_s"]), flush=True)
        if len(names) == 2:
            print("    indel / levenshtein rate: %.2f" % (out[-2]["gcells_per_s"] / out[-1]["gcells_per_s"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, type=int, metavar=("LO", "HI"))
    ap.add_argument("--metric", default="indel")
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    out = rates(((args.nx,) + tuple(args.one),), (args.metric,), 1) if args.one else rates(ROWS, ("indel", "levenshtein"), args.launches)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
