"""Rates of the weighted-Levenshtein kernel (csrc/wed.hip) beside ERP at dim 1 and unit-cost Levenshtein -- the table of DESIGN.md
3.14.

  python tools/wed_rates.py                     every row: 2000 random strings, all 1 999 000 pairs i < j in one launch, lengths
                                                20..60, 400..500 (the (8, 64) shape) and 450..550 (the (32, 64) shape), alphabets of 4, 26 and 128 symbols; "erp_pairs" on series of
                                                the same lengths, "levenshtein_pairs" on the same strings; one warm-up, then three
                                                launches, device events (Engine.last_kernel_ms), min .. max
  python tools/wed_rates.py --one A LO HI       one warm-up and one launch of one row: what a counter run wraps
  python tools/wed_rates.py --fit               the tests' 240-string fit (FIT_CFG) on the device and through the host path (the
                                                same recurrence as a Python callable in the worker pool), wall times
"""
import argparse
import json
import os
import string
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SYMBOLS = (string.ascii_lowercase + string.ascii_uppercase + string.digits + "".join(chr(k) for k in range(0x3b1, 0x3b1 + 66)))[:128]
FIT_CFG = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, niters=2)


def metric_costs(A, seed=2):
    """Random costs that are a metric: the shortest-path closure of random weights over the A symbols and the gap."""
    rng = np.random.default_rng(seed)
    W = np.triu(rng.uniform(0.3, 3.0, size=(A + 1, A + 1)), 1)
    D = W + W.T
    while True:
        before = D.copy()
        for c in range(A + 1):
            D = np.minimum(D, D[:, c, None] + D[None, c, :])
        if np.array_equal(D, before):
            return np.ascontiguousarray(D[:A, :A]), np.ascontiguousarray(D[:A, A])


def strings(nx, lo, hi, A, seed):
    rng = np.random.default_rng(seed)
    return ["".join(SYMBOLS[k] for k in rng.integers(0, A, size=int(L))) for L in rng.integers(lo, hi + 1, size=nx)]


def all_pairs(nx):
    i, j = np.triu_indices(nx, 1)
    return np.stack([i, j], axis=1).astype(np.int64)


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


def rates(nx, launches):
    from annchor_amd import distances

    IJ = all_pairs(nx)
    rows = []
    for lo, hi in ((20, 60), (400, 500), (450, 550)):
        rng = np.random.default_rng(lo)
        series = [np.cumsum(rng.standard_normal(int(L))) for L in rng.integers(lo, hi + 1, size=nx)]
        ms = timed(distances.erp, series, IJ, launches)
        rows.append(dict(kernel="erp_pairs", lengths=[lo, hi], A=None, ms=ms, cells=cells(series, IJ)))
        for A in (4, 26, 128):
            X = strings(nx, lo, hi, A, seed=A + lo)
            S, g = metric_costs(A)
            ms = timed(distances.WeightedLevenshtein(SYMBOLS[:A], S, g), X, IJ, launches)
            rows.append(dict(kernel="weighted_levenshtein_pairs", lengths=[lo, hi], A=A, ms=ms, cells=cells(X, IJ)))
            if A == 26:
                ms = timed(distances.levenshtein, X, IJ, launches)
                rows.append(dict(kernel="levenshtein_pairs", lengths=[lo, hi], A=A, ms=ms, cells=cells(X, IJ)))
    for r in rows:
        r["gcells_per_s"] = r["cells"] / (np.median(r["ms"]) * 1e-3) / 1e9
        print("%-28s lengths %3d..%3d  A %-4s  %9.2f .. %9.2f ms   %8.1f Gcell/s"
              % (r["kernel"], r["lengths"][0], r["lengths"][1], r["A"], min(r["ms"]), max(r["ms"]), r["gcells_per_s"]), flush=True)
    return rows


def wed_callable(x, y, S, g, at):
    """The definition as a host metric."""
    cx, cy = [at[ch] for ch in x], [at[ch] for ch in y]
    m = len(cy)
    prev = [0.0] * (m + 1)
    for j in range(m):
        prev[j + 1] = prev[j] + g[cy[j]]
    left = 0.0
    for a in cx:
        ga, Sa = g[a], S[a]
        left = left + ga
        cur = [left] * (m + 1)
        e = left
        for j in range(m):
            e = min(prev[j] + Sa[cy[j]], prev[j + 1] + ga, e + g[cy[j]])
            cur[j + 1] = e
        prev = cur
    return prev[m]


def fit_times():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import wed_cases as wc
    from annchor_amd import Annchor

    X, costs = wc.fit_strings(), wc.fit_costs()
    kw = wc.kwargs_of(costs)
    Annchor(X, "weighted_levenshtein", func_kwargs=kw, **FIT_CFG).fit()   # warm-up
    t = time.perf_counter()
    dev = Annchor(X, "weighted_levenshtein", func_kwargs=kw, **FIT_CFG).fit()
    t_dev = time.perf_counter() - t
    host_kw = dict(S=costs.S.tolist(), g=costs.g.tolist(), at={ch: a for a, ch in enumerate(costs.alphabet)})
    t = time.perf_counter()
    host = Annchor(X, wed_callable, func_kwargs=host_kw, **FIT_CFG).fit()
    t_host = time.perf_counter() - t
    same = bool(np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1]))
    print("fit of %d strings: device %.4f s (%d evaluations), host path %.2f s (%d evaluations), same graph distances: %s"
          % (len(X), t_dev, dev.evals, t_host, host.evals, same), flush=True)
    return dict(device_s=t_dev, host_s=t_host, evals=int(dev.evals), host_evals=int(host.evals), same=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, type=int, metavar=("A", "LO", "HI"))
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the rows as JSON here")
    args = ap.parse_args()
    if args.one:
        from annchor_amd import distances

        A, lo, hi = args.one
        S, g = metric_costs(A)
        ms = timed(distances.WeightedLevenshtein(SYMBOLS[:A], S, g), strings(args.nx, lo, hi, A, seed=A + lo), all_pairs(args.nx), 1)
        print("weighted_levenshtein_pairs A %d lengths %d..%d: %.2f ms" % (A, lo, hi, ms[0]), flush=True)
        return
    out = fit_times() if args.fit else rates(args.nx, args.launches)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
