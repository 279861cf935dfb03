"""The mutual-reachability spanning tree on the GPU (csrc/mst.hip, the reach form: k_mst_seed, k_mst_absorb<true>,
k_mst_classify_reach; Annchor / BruteForce .minimum_spanning_tree(min_samples), .hdbscan) against tests/mst_cases.py: Kruskal in
the order (w, i, j) over W = max(D, core[i], core[j]) of the dense brute-force matrix, core = the min_samples-th smallest entry
of a row.  Identical edges, bit-equal weights and core distances: no tolerances anywhere.  The fitted route runs where there is
something to fit: not two or three points, and not the 200 short strings, whose 7 distinct distances leave the fit's sampler
bins empty ("Some sampler bins contain too few samples"); those go through the seeded and the brute-force routes."""
import functools

import numpy as np
import pytest

import mst_cases as M

pytestmark = pytest.mark.gpu

NX = dict(pts2=2, pts3=3, pts130=130, strings=200, clusters=150, bundled320=320)
CASES = [(name, m, route) for name, nx in NX.items() for m in sorted({2, 3, 5, nx}) if m <= nx
         for route in ("fitted", "seeded", "brute") if route != "fitted" or name in ("pts130", "clusters", "bundled320")]


@functools.lru_cache(maxsize=None)
def reference(name, m):
    """(core, (edges, weights)) of the rule: computed once per case, shared, left unchanged."""
    D = M.case(name)[2]
    core = np.sort(D, axis=1)[:, m - 1]
    return core, M.kruskal(np.maximum(D, np.maximum(core[:, None], core[None, :])))


@functools.lru_cache(maxsize=None)
def annchor(name, fitted):
    """clusters: all three anchors in cluster 0, so a whole-cluster component has no anchor outside it (the cyclic bridge)."""
    from annchor_amd import Annchor
    from annchor_amd.pickers import SelectedAnchorPicker

    X, metric = M.case(name)[:2]
    kw = dict(n_anchors=3, anchor_picker=SelectedAnchorPicker([0, 1, 2])) if name == "clusters" else dict(n_anchors=min(5, len(X)))
    if name == "bundled320":
        kw = dict(n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2)
    ann = Annchor(X, metric, **{**dict(n_neighbors=5, n_samples=200, p_work=0.5, random_seed=7), **kw})
    return ann.fit() if fitted else ann


def poor_seed(nx, m):   # random indices, some outside 0..nx-1, some the row itself
    return np.random.default_rng(nx + m).integers(-3, nx + 3, size=(nx, m))


@pytest.mark.parametrize("name,m,route", CASES)
def test_reach_tree(name, m, route):
    core, want = reference(name, m)
    if route == "brute":
        obj = M.brute_force(*M.case(name)[:2])
        tree = obj.minimum_spanning_tree(min_samples=m)
    else:
        obj = annchor(name, route == "fitted")
        tree = obj.minimum_spanning_tree(min_samples=m, seed_graph=None if route == "fitted" else poor_seed(NX[name], m))
    print(name, m, route, "evals", obj.mst_evals, "core evals", obj.mst_core_evals, "per round", obj.mst_per_round)
    assert M.same_tree(tree, want)
    assert tree.min_samples == m and tree.core_distances.dtype == np.float64 and tree.core_distances.tobytes() == core.tobytes()
    assert obj.mst_rounds <= max(NX[name] - 1, 1).bit_length() and obj.mst_core_evals > 0


def test_min_samples_one_is_the_plain_tree():
    ann, bf = annchor("pts130", False), M.brute_force(*M.case("pts130")[:2])
    for tree, obj in ((ann.minimum_spanning_tree(min_samples=1), ann), (bf.minimum_spanning_tree(min_samples=1), bf)):
        assert M.same_tree(tree, M.case("pts130")[3]) and tree.core_distances is None and tree.min_samples == 1 and obj.mst_core_evals == 0


def test_several_ranges_per_round_give_the_same_tree():
    ann = annchor("pts130", False)
    assert M.same_tree(ann.minimum_spanning_tree(min_samples=5, seed_graph=poor_seed(130, 5), max_chunk_pairs=97), reference("pts130", 5)[1])
    assert ann.mst_chunks > ann.mst_rounds


def test_python_callable_metric_goes_through_fetch_and_edges():
    from annchor_amd import Annchor, BruteForce

    X, _, D, _ = M.case("pts130")
    core, want = reference("pts130", 5)

    def lookup(f, Xq, IJ):   # the object's evaluator answers from the host table
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return D[IJ[:, 0], IJ[:, 1]]

    def host_metric(a, b):
        raise AssertionError("not called one by one")

    ann = Annchor(list(X), host_metric, get_exact_ijs=lookup, n_anchors=5, n_neighbors=5, n_samples=200, p_work=0.5, random_seed=7)
    tree = ann.minimum_spanning_tree(min_samples=5, seed_graph=poor_seed(130, 5), max_chunk_pairs=300)
    assert M.same_tree(tree, want) and tree.core_distances.tobytes() == core.tobytes()
    assert M.same_tree(BruteForce(list(X), host_metric, get_exact_ijs=lookup).minimum_spanning_tree(min_samples=5), want)


def test_hdbscan_labels_are_the_host_extraction_of_the_reference_tree():
    from annchor_amd import radius

    core, want = reference("clusters", 5)
    labels, n = radius.hdbscan_labels(radius.SpanningTree(*want, 150, core, 5), 10)
    for res in (annchor("clusters", False).hdbscan(10, 5, seed_graph=poor_seed(150, 5)), M.brute_force(*M.case("clusters")[:2]).hdbscan(10, 5)):
        assert np.array_equal(res.labels, labels) and res.labels.dtype == np.int64 and res.n_clusters == n == 3
        assert res.n_noise == int((labels < 0).sum()) and (res.min_cluster_size, res.min_samples) == (10, 5) and M.same_tree(res.tree, want)
    assert [set(labels[a:a + 50][labels[a:a + 50] >= 0].tolist()) for a in (0, 50, 100)] == [{0}, {1}, {2}]


def test_argument_errors():
    ann, bf = annchor("pts130", False), M.brute_force(*M.case("pts130")[:2])
    for obj in (ann, bf):
        for bad in (0, 131, 2.0, True):
            with pytest.raises(ValueError, match=r"min_samples must be an integer in 1\.\.130 \(it counts the point itself\)"):
                obj.minimum_spanning_tree(min_samples=bad)
        with pytest.raises(ValueError, match=r"hdbscan: min_cluster_size must be an integer >= 2"):
            obj.hdbscan(min_cluster_size=1)
        with pytest.raises(ValueError, match=r"hdbscan: min_samples must be an integer in 1\.\.130"):
            obj.hdbscan(min_cluster_size=200)
