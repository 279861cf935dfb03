"""The rule of csrc/mst.hip restated (include/annchor_hip.h states it): the minimum spanning tree of the complete graph is what
Kruskal leaves when every pair i < j is taken in the strict order (distance bits ascending, i, j) -- distances as the metric
computes them for (smaller index, larger index) -- and the data sets of tests/test_mst_gpu.py."""
import functools

import numpy as np


def dense(bf):
    """The full distance matrix from a BruteForce object's complete rows."""
    idx, dist = bf.fit().neighbor_graph
    D = np.empty((bf.nx, bf.nx), dtype=np.float64)
    np.put_along_axis(D, np.asarray(idx, dtype=np.int64), np.asarray(dist, dtype=np.float64), axis=1)
    return D


def kruskal(D):
    """(edges int64 [nx - 1, 2], distances float64 [nx - 1]) of D's upper triangle, in the order they were taken."""
    nx = len(D)
    i, j = np.triu_indices(nx, k=1)
    d = np.ascontiguousarray(D[i, j], dtype=np.float64)
    assert not np.signbit(d).any() and not np.isnan(d).any()   # (then the bits of a distance order like its value)
    parent = list(range(nx))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    taken = []
    for t in np.lexsort((j, i, d.view(np.uint64))):
        a, b = find(i[t]), find(j[t])
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(t)
    taken = np.array(taken, dtype=np.int64)
    return np.stack([i[taken], j[taken]], axis=1).astype(np.int64).reshape(-1, 2), d[taken]


def same_tree(tree, want):
    return (tree.edges.dtype == np.int64 and tree.distances.dtype == np.float64 and tree.edges.shape == want[0].shape
            and np.array_equal(tree.edges, want[0]) and tree.distances.tobytes() == want[1].tobytes())


def _points(n, seed, dim=3):
    return np.random.default_rng(seed).standard_normal((n, dim))


def _strings():   # 200 strings of 1..6 symbols over {a, b}: at most 126 distinct ones, distances 0..6
    rng = np.random.default_rng(5)
    return np.array(["".join(rng.choice(["a", "b"], size=rng.integers(1, 7))) for _ in range(200)])


def _clusters():  # three far-apart clusters of 50 points, cluster 0 first: anchors 0, 1, 2 all lie in it
    rng = np.random.default_rng(9)
    return np.concatenate([rng.standard_normal((50, 2)) + c for c in ([0.0, 0.0], [40.0, 0.0], [0.0, 70.0])])


def _bundled():   # every fifth of the bundled strings
    from annchor_amd.datasets import load_strings

    return load_strings()["X"][::5]


def _host_euclidean(a, b):   # a Python callable: no device metric takes a single point
    return float(np.sqrt(((np.asarray(a) - np.asarray(b)) ** 2).sum()))


def host_pairs(f, X, IJ):
    return np.array([f(X[i], X[j]) for i, j in np.asarray(IJ).reshape(-1, 2)], dtype=np.float64)


DATA = {
    "bundled320": ("levenshtein", _bundled),
    "pts1": (_host_euclidean, lambda: list(_points(1, 1))), "pts2": ("euclidean", lambda: _points(2, 2)), "pts3": ("euclidean", lambda: _points(3, 3)),
    "pts130": ("euclidean", lambda: _points(130, 4)), "strings": ("levenshtein", _strings), "clusters": ("euclidean", _clusters),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, metric, dense matrix, (edges, distances) of the reference): computed once, shared, left unchanged."""
    metric, make = DATA[name]
    X = make()
    D = dense(brute_force(X, metric))
    return X, metric, D, kruskal(D)


def brute_force(X, metric):
    from annchor_amd import BruteForce

    return BruteForce(X, metric, get_exact_ijs=host_pairs if callable(metric) else None)
