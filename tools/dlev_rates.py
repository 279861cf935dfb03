"""Rates of the Damerau-Levenshtein kernel (csrc/dlev.hip, k_dlev) beside OSA.unit's (csrc/wed.hip, k_osa) and "levenshtein"'s
(csrc/lev.hip, bit-parallel) on the same strings -- the table of DESIGN.md 3.15c.

  python tools/dlev_rates.py          random strings over 26 symbols, all pairs i < j in one launch -- 2000 strings of 20..60
                                      symbols (the (8, 16) shape) and of 400..500 (the (8, 64) shape), 1000 strings of 900..1000
                                      (k_dlev: the (32, 64) shape; k_osa: its (16, 64)); one warm-up, then five launches, device
                                      events (Engine.last_kernel_ms), median and min .. max
  python tools/dlev_rates.py --fit    the tests' 160-string data set fitted (is_metric=True) on the device and through the host
                                      path (the same recurrence as a Python callable in the worker pool), wall times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wed_rates import FIT_CFG, SYMBOLS, all_pairs, cells, strings, timed   # noqa: E402  (adds the repository to sys.path)

A = 26
ROWS = ((2000, 20, 60), (2000, 400, 500), (1000, 900, 1000))


def rates(launches):
    from annchor_amd import distances

    rows = []
    for nx, lo, hi in ROWS:
        IJ = all_pairs(nx)
        X = strings(nx, lo, hi, A, seed=A + lo)
        n = cells(X, IJ)
        for kernel, metric in (("damerau_levenshtein_pairs", distances.damerau_levenshtein), ("osa_pairs", distances.OSA.unit(SYMBOLS[:A])),
                               ("levenshtein", distances.levenshtein)):
            ms = timed(metric, X, IJ, launches)
            rows.append(dict(kernel=kernel, nx=nx, lengths=[lo, hi], A=A, ms=ms, cells=n, gcells_per_s=n / (np.median(ms) * 1e-3) / 1e9))
            print("%-26s %4d strings of %3d..%4d  median %9.3f ms  (%9.3f .. %9.3f)   %9.1f Gcell/s"
                  % (kernel, nx, lo, hi, np.median(ms), min(ms), max(ms), rows[-1]["gcells_per_s"]), flush=True)
        print("    damerau_levenshtein / osa rate: %.2f;  levenshtein / damerau_levenshtein rate: %.1f"
              % (rows[-3]["gcells_per_s"] / rows[-2]["gcells_per_s"], rows[-1]["gcells_per_s"] / rows[-3]["gcells_per_s"]), flush=True)
    return rows


def fit_times():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import dlev_cases as dc
    import osa_cases as oc
    from annchor_amd import Annchor

    X = oc.mutated_strings(160, 20, 45, 12, seed=5)
    Annchor(X, dc.NAME, **FIT_CFG).fit()   # warm-up
    t = time.perf_counter()
    dev = Annchor(X, dc.NAME, **FIT_CFG).fit()
    t_dev = time.perf_counter() - t
    t = time.perf_counter()
    host = Annchor(X, dc.dl_loop, **FIT_CFG).fit()
    t_host = time.perf_counter() - t
    same = bool(np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1]))
    print("fit of %d strings: device %.4f s (%d evaluations), host path %.2f s (%d evaluations), same graph distances: %s"
          % (len(X), t_dev, dev.evals, t_host, host.evals, same), flush=True)
    return dict(device_s=t_dev, host_s=t_host, evals=int(dev.evals), host_evals=int(host.evals), same=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    out = fit_times() if args.fit else rates(args.launches)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
