"""Times Annchor.dbscan against the route to the same labels without it: radius_graph(eps, mode="connectivity")
followed by the host reference's clustering of its CSR (tests/dbscan_cases.py).

    python tools/dbscan_timing.py [--n 8000] [--eps 19] [--min-samples 5] [--anchors 20] [--runs 5]

Host clock around whole calls (each ends in a device wait), the routes alternating, `runs` runs after a warm-up, median
(min-max); then one profiled run of its own for the per-scope device times.  The anchors are picked before anything is timed.
Prints one JSON line per figure.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _stat(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(ts.min()), 3), max_ms=round(float(ts.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--eps", type=float, default=19.0)
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--anchors", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()

    import dbscan_cases as DC
    from annchor_amd import Annchor
    from annchor_amd.datasets import synthetic_string_clusters

    X = synthetic_string_clusters(a.n)
    ann = Annchor(X, "levenshtein", n_anchors=a.anchors, n_neighbors=15, random_seed=1)
    ann.get_anchors()

    def route_dbscan():
        return ann.dbscan(a.eps, a.min_samples)

    def route_graph():
        return ann.radius_graph(a.eps, mode="connectivity")

    def host_cluster(g):
        return DC.reference(ann.nx, DC.edges_of_csr(g.indptr, g.indices), a.min_samples)

    res, g = route_dbscan(), route_graph()   # warm-up of both routes
    labels, core, ncl = host_cluster(g)
    same = bool(np.array_equal(res.labels, labels) and np.array_equal(res.core_sample_mask, core) and res.n_clusters == ncl)
    print(json.dumps(dict(what="case", n=a.n, eps=a.eps, min_samples=a.min_samples, anchors=a.anchors, edges=ann.dbscan_edges,
                          evals=ann.dbscan_evals, radius_evals=ann.radius_evals, sure=ann.dbscan_sure, pruned=ann.dbscan_pruned,
                          clusters=res.n_clusters, noise=res.n_noise, core=int(res.core_sample_mask.sum()),
                          labels_equal_host_route=same)))
    if not same:
        raise SystemExit("dbscan() and the host route disagree")
    t_db, t_graph, t_host = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        route_dbscan()
        t1 = time.perf_counter()
        g = route_graph()
        t2 = time.perf_counter()
        host_cluster(g)
        t3 = time.perf_counter()
        t_db.append(t1 - t0)
        t_graph.append(t2 - t1)
        t_host.append(t3 - t2)
    print(json.dumps(dict(what="Annchor.dbscan", **_stat(t_db))))
    print(json.dumps(dict(what="radius_graph(connectivity)", **_stat(t_graph))))
    print(json.dumps(dict(what="host reference clustering of the CSR", **_stat(t_host))))

    eng = ann._engine
    for name, fn in (("Annchor.dbscan", route_dbscan), ("radius_graph(connectivity)", route_graph)):
        eng.prof_enable(1)
        eng.prof_reset()
        fn()
        prof = {k: v for k, v in eng.prof_get().items() if v["launches"]}
        eng.prof_enable(0)
        print(json.dumps(dict(what="device scopes of one profiled " + name, total_ms=round(sum(v["ms"] for v in prof.values()), 4),
                              dbscan_kernels_ms=round(sum(v["ms"] for k, v in prof.items() if k.startswith("dbscan_")), 4),
                              scopes={k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in sorted(prof.items())})))


if __name__ == "__main__":
    main()
