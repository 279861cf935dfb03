"""Rates of the optimal-string-alignment kernel (csrc/wed.hip, k_osa) beside weighted Levenshtein's on the same strings and table
-- the table of DESIGN.md 3.15b.

  python tools/osa_rates.py          every row: random strings, all pairs i < j in one launch -- 2000 strings of 20..60 symbols
                                     (the (8, 16) shape) and of 400..500 (the (8, 64) shape), 1000 strings of 900..1000 (osa: the
                                     (16, 64) shape; weighted Levenshtein: its (32, 64)) -- alphabets of 4, 26 and 128 symbols,
                                     transpose = 0.2 (below every other cost: swaps win wherever the strings allow one) and
                                     transpose = +inf (none does); one warm-up, then three launches, device events
                                     (Engine.last_kernel_ms), min .. max
  python tools/osa_rates.py --fit    the tests' 240-string fit (FIT_CFG, is_metric=False) on the device and through the host path
                                     (the same recurrence as a Python callable in the worker pool), wall times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wed_rates import FIT_CFG, SYMBOLS, all_pairs, cells, metric_costs, strings, timed   # noqa: E402  (adds the repository to sys.path)

TRANSPOSE = 0.2
ROWS = ((2000, 20, 60), (2000, 400, 500), (1000, 900, 1000))


def rates(launches):
    from annchor_amd import distances

    rows = []
    for nx, lo, hi in ROWS:
        IJ = all_pairs(nx)
        for A in (4, 26, 128):
            X = strings(nx, lo, hi, A, seed=A + lo)
            S, g = metric_costs(A)
            n = cells(X, IJ)
            for kernel, T, metric in (("weighted_levenshtein_pairs", None, distances.WeightedLevenshtein(SYMBOLS[:A], S, g)),
                                      ("osa_pairs", TRANSPOSE, distances.OSA(SYMBOLS[:A], S, g, TRANSPOSE)),
                                      ("osa_pairs", float("inf"), distances.OSA(SYMBOLS[:A], S, g, float("inf")))):
                ms = timed(metric, X, IJ, launches)
                rows.append(dict(kernel=kernel, transpose=T, nx=nx, lengths=[lo, hi], A=A, ms=ms, cells=n,
                                 gcells_per_s=n / (np.median(ms) * 1e-3) / 1e9))
                r = rows[-1]
                print("%-28s T %-5s %4d strings of %3d..%4d  A %-4d  %9.2f .. %9.2f ms   %8.1f Gcell/s"
                      % (kernel, "-" if T is None else T, nx, lo, hi, A, min(ms), max(ms), r["gcells_per_s"]), flush=True)
            print("    osa / weighted Levenshtein rate: %.2f (transpose %s), %.2f (transpose inf)"
                  % (rows[-2]["gcells_per_s"] / rows[-3]["gcells_per_s"], TRANSPOSE, rows[-1]["gcells_per_s"] / rows[-3]["gcells_per_s"]),
                  flush=True)
    return rows


def osa_callable(x, y, S, g, T, at):
    """The definition as a host metric."""
    cx, cy = [at[ch] for ch in x], [at[ch] for ch in y]
    m = len(cy)
    prev = [0.0] * (m + 1)
    for j in range(m):
        prev[j + 1] = prev[j] + g[cy[j]]
    prev2 = None
    left = 0.0
    for i, a in enumerate(cx):
        ga, Sa = g[a], S[a]
        left = left + ga
        cur = [left] * (m + 1)
        e = left
        for j in range(m):
            b = cy[j]
            e = min(prev[j] + Sa[b], prev[j + 1] + ga, e + g[b])
            if i >= 1 and j >= 1 and a == cy[j - 1] and cx[i - 1] == b:
                e = min(e, prev2[j - 1] + T)
            cur[j + 1] = e
        prev2, prev = prev, cur
    return prev[m]


def fit_times():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import osa_cases as oc
    from annchor_amd import Annchor

    X, costs = oc.fit_strings(), oc.fit_costs()
    kw = oc.kwargs_of(costs)
    Annchor(X, "osa", func_kwargs=kw, is_metric=False, **FIT_CFG).fit()   # warm-up
    t = time.perf_counter()
    dev = Annchor(X, "osa", func_kwargs=kw, is_metric=False, **FIT_CFG).fit()
    t_dev = time.perf_counter() - t
    host_kw = dict(S=costs.S.tolist(), g=costs.g.tolist(), T=costs.T, at={ch: a for a, ch in enumerate(costs.alphabet)})
    t = time.perf_counter()
    host = Annchor(X, osa_callable, func_kwargs=host_kw, is_metric=False, **FIT_CFG).fit()
    t_host = time.perf_counter() - t
    same = bool(np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1]))
    print("fit of %d strings: device %.4f s (%d evaluations), host path %.2f s (%d evaluations), same graph distances: %s"
          % (len(X), t_dev, dev.evals, t_host, host.evals, same), flush=True)
    return dict(device_s=t_dev, host_s=t_host, evals=int(dev.evals), host_evals=int(host.evals), same=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    out = fit_times() if args.fit else rates(args.launches)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
