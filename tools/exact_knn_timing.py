"""Times Annchor.exact_neighbor_graph() after fit() against BruteForce.fit(k) on the same data, and against fit() alone
(DESIGN.md 3.22): what the certificate of a fit costs.

    python tools/exact_knn_timing.py [--n 8000] [--anchors 20] [--k 15] [--runs 5]      # clustered strings
    python tools/exact_knn_timing.py --bundled [--runs 5]                               # the 1600 bundled strings at C2

Host clock around whole calls (each ends in a device wait), the routes alternating, `runs` runs after a warm-up, median
(min-max); then one profiled run of its own for the per-scope device times, grouped into seed evaluation, classify,
evaluation, absorb and finish.  k is the fit's own and the seed is the fit's graph.  Prints one JSON line per figure.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(ts.min()), 3), max_ms=round(float(ts.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--anchors", type=int, default=20)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bundled", action="store_true", help="the 1600 bundled strings at n_anchors=15, k=25, p_work=0.12")
    a = ap.parse_args()

    from annchor_amd import Annchor, BruteForce, compare_neighbor_graphs
    from annchor_amd.datasets import load_strings, synthetic_string_clusters

    if a.bundled:
        X, cfg, what = load_strings()["X"], dict(n_anchors=15, n_neighbors=25, p_work=0.12, random_seed=42), "bundled strings, C2"
    else:
        X, cfg = synthetic_string_clusters(a.n), dict(n_anchors=a.anchors, n_neighbors=a.k, random_seed=1)
        what = "%d clustered strings, %d anchors" % (a.n, a.anchors)
    k = cfg["n_neighbors"]

    def route_fit():
        return Annchor(X, "levenshtein", **cfg).fit()

    def route_exact(ann):
        return ann.exact_neighbor_graph()

    bf = BruteForce(X, "levenshtein")

    def route_brute():
        return bf.fit(k).neighbor_graph

    ann = route_fit()                     # warm-up of all three routes
    exact, want = route_exact(ann), route_brute()
    same = bool(np.array_equal(exact[0], want[0]) and exact[1].tobytes() == want[1].tobytes())
    print(json.dumps(dict(what="case", data=what, nx=len(X), k=k, fit_errors=int(compare_neighbor_graphs(exact, ann.neighbor_graph, k)),
                          cells=len(X) * k, pairs=ann.exact_pairs, evals=ann.exact_evals, share_evaluated=round(ann.exact_evals / ann.exact_pairs, 4),
                          seed_evals=ann.exact_seed_evals, entries=ann.exact_entries, chunks=ann.exact_chunks, inf_rows=ann.exact_inf_rows,
                          equals_brute_force=same)))
    if not same:
        raise SystemExit("exact_neighbor_graph() and BruteForce.fit() disagree")
    t_fit, t_exact, t_brute = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        ann = route_fit()
        t1 = time.perf_counter()
        route_exact(ann)
        t2 = time.perf_counter()
        route_brute()
        t3 = time.perf_counter()
        t_fit.append(t1 - t0)
        t_exact.append(t2 - t1)
        t_brute.append(t3 - t2)
    print(json.dumps(dict(what="Annchor(...).fit() (constructor included)", **_stat(t_fit))))
    print(json.dumps(dict(what="exact_neighbor_graph() after fit()", **_stat(t_exact))))
    print(json.dumps(dict(what="BruteForce.fit(k)", **_stat(t_brute))))

    eng = ann._engine
    eng.prof_enable(1)
    eng.prof_reset()
    route_exact(ann)
    prof = {n: v for n, v in eng.prof_get().items() if v["launches"]}
    eng.prof_enable(0)

    def ms(pred):
        return round(sum(v["ms"] for n, v in prof.items() if pred(n)), 4)

    # (the metric kernels' scopes end in "_pairs": the seed entries and the walk's candidates both run through them)
    print(json.dumps(dict(what="device scopes of one profiled exact_neighbor_graph()", total_ms=round(sum(v["ms"] for v in prof.values()), 4),
                          classify_ms=ms(lambda n: n == "knn_exact_classify"), metric_ms=ms(lambda n: n.endswith("_pairs")),
                          scan_emit_ms=ms(lambda n: n in ("knn_exact_emit", "exclusive_scan")), absorb_ms=ms(lambda n: n == "knn_exact_absorb"),
                          finish_ms=ms(lambda n: n in ("knn_exact_scatter", "knn_exact_rows")),
                          scopes={n: dict(ms=round(v["ms"], 4), launches=v["launches"]) for n, v in sorted(prof.items())})))
    # the seed evaluation on its own: the radii of the fit's graph, host clock (one metric call and the NumPy around it)
    from annchor_amd import radius

    ts = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        radius.seed_radii(ann.nx, k, ann.neighbor_graph[0], lambda IJ: ann.get_exact_ijs(ann.f, ann.X, IJ))
        ts.append(time.perf_counter() - t0)
    print(json.dumps(dict(what="seed radii alone (host clock)", **_stat(ts))))


if __name__ == "__main__":
    main()
