"""Times Annchor.minimum_spanning_tree() -- seeded by a fit, and unseeded -- against BruteForce.minimum_spanning_tree() on the
same data, with BruteForce.fit(15) as the cost of one pass over all pairs.

    python tools/mst_timing.py [--n 8000] [--anchors 20] [--runs 5]      # clustered strings
    python tools/mst_timing.py --bundled [--runs 5]                      # the 1600 bundled strings at C2
    python tools/mst_timing.py [--bundled] --min-samples 5               # the mutual-reachability tree

With --min-samples m >= 2 the routes are minimum_spanning_tree(min_samples=m) from a fitted object and from BruteForce, the plain
tree of the same fitted object, and the k-NN step alone on either side (exact_neighbor_graph(m), BruteForce.fit(m)).

Host clock around whole calls (each ends in a device wait), the routes alternating, `runs` runs after a warm-up, median
(min-max); then one profiled call of each bounded route for the per-scope device times, and the evaluations and pool size per
round.  Prints one JSON line per figure.  Needs a GPU."""
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bundled", action="store_true", help="the 1600 bundled strings at n_anchors=15, k=25, p_work=0.12")
    ap.add_argument("--min-samples", type=int, default=1, help="m >= 2: mutual-reachability weights from the m-th smallest row entries")
    a = ap.parse_args()
    m = a.min_samples

    from annchor_amd import Annchor, BruteForce
    from annchor_amd.datasets import load_strings, synthetic_string_clusters

    if a.bundled:
        X, cfg, what = load_strings()["X"], dict(n_anchors=15, n_neighbors=25, p_work=0.12, random_seed=42), "bundled strings, C2"
    else:
        X, cfg = synthetic_string_clusters(a.n), dict(n_anchors=a.anchors, n_neighbors=15, random_seed=1)
        what = "%d clustered strings, %d anchors" % (a.n, a.anchors)

    fitted = Annchor(X, "levenshtein", **cfg).fit()
    bare = Annchor(X, "levenshtein", **cfg)
    bare.get_anchors()
    bf = BruteForce(X, "levenshtein")
    if m >= 2:
        routes = [("minimum_spanning_tree(min_samples=%d) from a fitted object" % m, lambda: fitted.minimum_spanning_tree(min_samples=m)),
                  ("BruteForce.minimum_spanning_tree(min_samples=%d)" % m, lambda: bf.minimum_spanning_tree(min_samples=m)),
                  ("minimum_spanning_tree() seeded by the fit", fitted.minimum_spanning_tree),
                  ("exact_neighbor_graph(%d) from the fit" % m, lambda: fitted.exact_neighbor_graph(m)),
                  ("BruteForce.fit(%d)" % m, lambda: bf.fit(m))]
        reach, brute = routes[0][1](), routes[1][1]()                 # warm-up; the statistics below are these calls'
        same = np.array_equal(reach.edges, brute.edges) and reach.distances.tobytes() == brute.distances.tobytes()
        for name, obj in (("fitted", fitted), ("brute force", bf)):
            print(json.dumps(dict(what="case", route=name, data=what, nx=len(X), min_samples=m, pairs=obj.mst_pairs, evals=obj.mst_evals,
                                  core_evals=obj.mst_core_evals, evals_per_pair=round(obj.mst_evals / obj.mst_pairs, 4), rounds=obj.mst_rounds,
                                  pool=obj.mst_pool, chunks=obj.mst_chunks, per_round_evals_pool=obj.mst_per_round, equals_brute_force=same)))
        if not same:
            raise SystemExit("the routes disagree")
        for _, call in routes[2:]:
            call()
        fitted.minimum_spanning_tree()
        print(json.dumps(dict(what="case", route="plain tree, fitted", evals=fitted.mst_evals, rounds=fitted.mst_rounds, pool=fitted.mst_pool,
                              per_round_evals_pool=fitted.mst_per_round)))
        _time(routes, a.runs)
        _profile([("fitted, min_samples=%d" % m, fitted, lambda: fitted.minimum_spanning_tree(min_samples=m))])
        return
    routes = [("minimum_spanning_tree() seeded by the fit", fitted.minimum_spanning_tree),
              ("minimum_spanning_tree() unseeded", bare.minimum_spanning_tree),
              ("BruteForce.minimum_spanning_tree()", bf.minimum_spanning_tree),
              ("BruteForce.fit(15)", lambda: bf.fit(15))]
    trees = [call() for _, call in routes][:3]                     # warm-up of every route
    same = all(np.array_equal(t.edges, trees[2].edges) and t.distances.tobytes() == trees[2].distances.tobytes() for t in trees)
    for name, obj in (("seeded", fitted), ("unseeded", bare), ("brute force", bf)):
        print(json.dumps(dict(what="case", route=name, data=what, nx=len(X), pairs=obj.mst_pairs, evals=obj.mst_evals,
                              evals_per_pair=round(obj.mst_evals / obj.mst_pairs, 4), rounds=obj.mst_rounds, pool=obj.mst_pool,
                              chunks=obj.mst_chunks, per_round_evals_pool=obj.mst_per_round, equals_brute_force=same)))
    if not same:
        raise SystemExit("the routes disagree")
    _time(routes, a.runs)
    _profile([("seeded", fitted, fitted.minimum_spanning_tree), ("unseeded", bare, bare.minimum_spanning_tree)])


def _time(routes, runs):
    times = [[] for _ in routes]
    for _ in range(runs):
        for ts, (_, call) in zip(times, routes):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
    for ts, (name, _) in zip(times, routes):
        print(json.dumps(dict(what=name, **_stat(ts))))


def _profile(cases):
    for name, obj, call in cases:
        eng = obj._engine
        eng.prof_enable(1)
        eng.prof_reset()
        call()
        prof = {n: v for n, v in eng.prof_get().items() if v["launches"]}
        eng.prof_enable(0)
        print(json.dumps(dict(what="device scopes of one profiled call", route=name, total_ms=round(sum(v["ms"] for v in prof.values()), 4),
                              scopes={n: dict(ms=round(v["ms"], 4), launches=v["launches"]) for n, v in sorted(prof.items())})))


if __name__ == "__main__":
    main()
