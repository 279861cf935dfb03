"""DBSCAN on the host: the rule restated in plain Python / NumPy, the edge-list cases of the kernel tests, the injected anchor
table of the absorb test and the parameters of the end-to-end tests.

The rule (include/annchor_hip.h; scikit-learn's DBSCAN made order-free), for nx points and a set of undirected edges:
    core(i)    iff degree(i) + 1 >= min_samples          (the neighbourhood of i includes i)
    clusters   the connected components of the core-core edges, numbered 0, 1, ... by ascending smallest core index
    border     a non-core point with a core neighbour takes the smallest cluster number among its core neighbours
    noise      every other point: -1
`reference` is a sequential union-find; tests/test_dbscan_cases.py checks it against sklearn.cluster.DBSCAN.

Every case is small enough to run in milliseconds and is kept at the size at which a kernel can still go wrong: point counts on
the wavefront and workgroup edges, a path that is one long chain of hooks, a hub whose word every lane hits, bridges that must
not merge clusters.  The module asserts at import that the cases together hold what the tests claim to cover (CONDITIONS)."""
import numpy as np


# ------------------------------------------------------------------------------------------------------ the reference
def reference(nx, edges, min_samples):
    """(labels int64 [nx], core bool [nx], n_clusters).  edges: int [n, 2], each unordered pair once, either orientation."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    deg = np.bincount(edges.ravel(), minlength=nx)[:nx] if len(edges) else np.zeros(nx, dtype=np.int64)
    core = deg + 1 >= min_samples
    parent = list(range(nx))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for i, j in edges.tolist():
        if core[i] and core[j]:
            a, b = find(i), find(j)
            if a != b:
                parent[b] = a            # (any orientation: the numbering below does not rely on which root survives)
    root = np.array([find(v) if core[v] else -1 for v in range(nx)], dtype=np.int64)
    labels = np.full(nx, -1, dtype=np.int64)
    n_clusters = 0
    if core.any():
        # number the components by their smallest core index
        smallest = np.full(nx, nx, dtype=np.int64)
        cidx = np.flatnonzero(core)
        np.minimum.at(smallest, root[cidx], cidx)
        order = np.sort(smallest[smallest < nx])
        n_clusters = len(order)
        labels[cidx] = np.searchsorted(order, smallest[root[cidx]])
    big = np.iinfo(np.int64).max
    best = np.full(nx, big, dtype=np.int64)
    for a, b in ((0, 1), (1, 0)):
        c, o = edges[:, a], edges[:, b]
        m = core[c] & ~core[o]
        np.minimum.at(best, o[m], labels[c[m]])
    border = best < big
    labels[border] = best[border]
    return labels, core, n_clusters


def edges_of_csr(indptr, indices):
    """Upper-triangle edges (i < j) of a symmetric CSR (RadiusGraph.indptr / indices, or radius_cases.graph_from_matrix)."""
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    keep = rows < indices
    return np.stack([rows[keep], np.asarray(indices, dtype=np.int64)[keep]], axis=1)


def census(nx, edges, min_samples):
    """What a case holds, on the host reference: the counts the conditions below and the end-to-end tests are stated in."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    labels, core, ncl = reference(nx, edges, min_samples)
    nclu = np.zeros(nx, dtype=np.int64)     # per non-core point: distinct clusters among its core neighbours
    seen = set()
    for i, j in edges.tolist():
        for c, o in ((i, j), (j, i)):
            if core[c] and not core[o] and (o, labels[c]) not in seen:
                seen.add((o, labels[c]))
                nclu[o] += 1
    # a component whose smallest core index is not an end point of its first core-core edge (in the order given)
    late_root = False
    first = {}
    for i, j in edges.tolist():
        if core[i] and core[j] and labels[i] not in first:
            first[labels[i]] = (i, j)
    for lab, (i, j) in first.items():
        smallest = int(np.flatnonzero(core & (labels == lab))[0])
        late_root |= smallest not in (i, j)
    return dict(clusters=int(ncl), noise=int((labels < 0).sum()), border=int(((labels >= 0) & ~core).sum()),
                multi_border=int((nclu >= 2).sum()), late_root=bool(late_root))


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(nx, edges, min_samples, batches=None, group=None):
    """batches: how the edge list is cut for dbscan_edges (sizes; None: one call); group: cases of one group are the same
    graph in different edge orders and must give identical arrays."""
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    return dict(nx=int(nx), edges=edges, min_samples=int(min_samples), batches=batches, group=group)


def _clique(nodes):
    nodes = list(nodes)
    return [(a, b) for k, a in enumerate(nodes) for b in nodes[k + 1:]]


def _geometric(n, mean_degree, seed):
    """Random geometric graph: n uniform points in the unit square (their numbering is random by construction), an edge below
    the distance that gives the wanted mean degree."""
    rng = np.random.default_rng(seed)
    P = rng.random((n, 2))
    r2 = mean_degree / (np.pi * n)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    i, j = np.nonzero(np.triu(d2 <= r2, k=1))
    return np.stack([i, j], axis=1)


CASES = {}
for _nx in (1, 2, 63, 64, 65, 257):                       # no edges: nx on the wavefront and workgroup edges
    CASES["empty%d_ms1" % _nx] = _case(_nx, [], 1)         # every point a singleton cluster
    CASES["empty%d_ms2" % _nx] = _case(_nx, [], 2)         # all noise

# a path of 4096 nodes (min_samples 3: the inner nodes are core and one component, the two ends are border points): deep
# finds and contended hooks.  Three numberings of the nodes x three orders of the edge list.
_PATH = 4096
_rng = np.random.default_rng(11)
_numberings = {"id": np.arange(_PATH), "rev": np.arange(_PATH)[::-1].copy(), "perm": _rng.permutation(_PATH)}
_shuffle = _rng.permutation(_PATH - 1)
for _nn, _num in _numberings.items():
    _e = np.stack([_num[:-1], _num[1:]], axis=1)
    CASES["path_%s_asc" % _nn] = _case(_PATH, _e, 3, group="path_" + _nn)
    CASES["path_%s_desc" % _nn] = _case(_PATH, _e[::-1], 3, group="path_" + _nn)
    CASES["path_%s_shuffled" % _nn] = _case(_PATH, _e[_shuffle], 3, group="path_" + _nn)

# a star with 300 leaves around point 150: every leaf edge adds to one degree word and hooks under or over one root
_leaves = [v for v in range(301) if v != 150]
_star = [(150, v) if v % 2 else (v, 150) for v in _leaves]
CASES["star_ms2"] = _case(301, _star, 2)                  # everything core, one cluster
CASES["star_ms301"] = _case(301, _star, 301)              # the hub alone is core: 300 border points take its number
CASES["star_ms302"] = _case(301, _star, 302)              # nothing is core: all noise

# two 5-cliques {1..5} and {6..10} joined only through point 0 (degree 2, not core at min_samples 5): two clusters, and the
# bridge takes the lower number -- also when the higher clique's edge to it comes first
_two = _clique(range(1, 6)) + _clique(range(6, 11))
CASES["bridge"] = _case(11, _two + [(0, 3), (0, 8)], 5, group="bridge")
CASES["bridge_high_first"] = _case(11, [(8, 0), (3, 0)] + _two[::-1], 5, group="bridge")

# a non-core point (15) adjacent to three clusters, the highest-numbered one first
_three = _clique(range(0, 5)) + _clique(range(5, 10)) + _clique(range(10, 15))
CASES["three_clusters"] = _case(16, [(15, 12), (7, 15), (15, 1)] + _three, 5)

# min_samples 1: every point is core, isolated points are singleton clusters, no noise
_sparse = np.random.default_rng(12).integers(0, 100, (40, 2))
_sparse = np.unique(np.sort(_sparse[_sparse[:, 0] != _sparse[:, 1]], axis=1), axis=0)
CASES["ms1"] = _case(100, _sparse, 1)
CASES["ms_above_all"] = _case(100, _sparse, 1000)          # min_samples above every degree + 1: all noise
CASES["complete65"] = _case(65, _clique(range(65)), 65)    # degree 64 everywhere: all core at 65
CASES["complete65_noise"] = _case(65, _clique(range(65)), 66)

# 2000 points, about 25 000 edges; the 7-batch form grows the device edge list across absorbs (one batch is empty)
_G = _geometric(2000, 26.5, 13)                             # (26.5 before the square's border takes its share: 24 921 edges)
_G = _G[np.random.default_rng(14).permutation(len(_G))]
_G[::2] = _G[::2, ::-1]                                     # both orientations
for _ms in (3, 10, 20, 30):                                 # (30: the core points fall apart into many clusters)
    CASES["random_ms%d" % _ms] = _case(2000, _G, _ms, group="random_ms10" if _ms == 10 else None)
_sizes = [5000, 1, 0, 9000, 37, 4096]
CASES["random_ms10_batches"] = _case(2000, _G, 10, batches=_sizes + [len(_G) - sum(_sizes)], group="random_ms10")
assert 24000 < len(_G) < 26000 and len(_G) - sum(_sizes) > 0


def batches(name):
    """The case's edge list cut into the arrays its dbscan_edges calls take."""
    c = CASES[name]
    if c["batches"] is None:
        return [c["edges"]]
    cuts = np.cumsum([0] + list(c["batches"]))
    assert cuts[-1] == len(c["edges"])
    return [c["edges"][a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# the reference of every case, computed once and never written
REFERENCE = {}
CENSUS = {}
for _name, _c in CASES.items():
    _lab, _core, _ncl = reference(_c["nx"], _c["edges"], _c["min_samples"])
    _lab.setflags(write=False)
    _core.setflags(write=False)
    REFERENCE[_name] = (_lab, _core, _ncl)
    CENSUS[_name] = census(_c["nx"], _c["edges"], _c["min_samples"])

# What the cases must contain, on the host reference -- conditions, not measurements.
CONDITIONS = {
    "two clusters in one case": any(s["clusters"] >= 2 for s in CENSUS.values()),
    "noise": any(s["noise"] > 0 for s in CENSUS.values()),
    "a border point": any(s["border"] > 0 for s in CENSUS.values()),
    "a border point with core neighbours in two or more clusters": any(s["multi_border"] > 0 for s in CENSUS.values()),
    "a component whose smallest core index is not its first edge's end point": any(s["late_root"] for s in CENSUS.values()),
}
assert all(CONDITIONS.values()), [k for k, v in CONDITIONS.items() if not v]


# ----------------------------------------------------------------------------- injected anchor table (the absorb test)
def sure_or_out_table(seed=5):
    """Points on a line in tight groups of sizes 1 .. 12, one anchor at every group's centre, the points shuffled: float64
    [nx, na].  At r = 3, rtol = 0 every pair of one group is SURE (both within 1 of their own anchor: s + t <= 2 < 3) and every
    pair across groups is OUT (the groups are 100 apart), so the connectivity-mode lists hold no candidate and the graph is a
    union of cliques.  Returns (D, r)."""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 3, 4, 5, 6, 7, 9, 12, 64, 70]
    centre = np.repeat(100.0 * np.arange(len(sizes)), sizes)
    x = centre + rng.integers(-1, 2, len(centre))
    x = x[rng.permutation(len(x))]
    D = np.abs(x[:, None] - 100.0 * np.arange(len(sizes))[None, :])
    return np.ascontiguousarray(D, dtype=np.float64), 3.0


# -------------------------------------------------------------------------------------------- end-to-end parameters
# eps and min_samples per data set of the end-to-end test, chosen on the host double-loop matrix so that the reference shows
# at least 2 clusters, 1 noise point and 1 border point (tests/test_dbscan_gpu.py states the counts obtained).
E2E = {
    "levenshtein": dict(eps=8.0, min_samples=10),      # radius_cases.clustered_strings(300)
    "euclidean_f64": dict(eps=4.0, min_samples=10),    # radius_cases.lattice_points(260, 5, 5, float64): 4.0 is an attained distance
}
