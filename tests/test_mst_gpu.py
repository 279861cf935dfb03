"""The minimum spanning tree on the GPU (csrc/mst.hip, annchor_amd/radius.py: spanning_tree, Annchor / BruteForce
.minimum_spanning_tree) against tests/mst_cases.py: Kruskal in the order (distance, i, j) over the dense brute-force matrix.
Identical edge arrays and bit-equal distances: no tolerances anywhere."""
import numpy as np
import pytest

import mst_cases as M

pytestmark = pytest.mark.gpu

CFG = dict(n_neighbors=5, n_samples=200, p_work=0.5, random_seed=7)


def _ann(name, **kw):
    from annchor_amd import Annchor

    X, metric, _, want = M.case(name)
    return Annchor(X, metric, **{**CFG, "n_anchors": min(5, len(X)), **kw}), want


@pytest.mark.parametrize("name", ["pts1", "pts2", "pts3", "pts130", "strings", "clusters"])
def test_brute_force_tree(name):
    X, metric, _, want = M.case(name)
    bf = M.brute_force(X, metric)
    tree = bf.minimum_spanning_tree()
    assert M.same_tree(tree, want) and tree.nx == len(X) and len(tree.edges) == len(X) - 1
    assert bf.mst_rounds <= max(len(X) - 1, 0).bit_length() and bf.mst_pairs == len(X) * (len(X) - 1) // 2


@pytest.mark.parametrize("name", ["pts2", "pts3", "pts130", "strings"])
def test_bounded_tree(name):
    """Two and three points; two row blocks and a 64-column chunk edge at the default bound_rtol of a float metric; strings
    with many duplicates and equal distances (the tie rule, zero-weight edges, mutual picks)."""
    ann, want = _ann(name)
    tree = ann.minimum_spanning_tree()
    assert M.same_tree(tree, want)
    assert ann.evals == ann.n_anchors * ann.nx + ann.mst_evals and ann.mst_pairs == ann.nx * (ann.nx - 1) // 2
    if name == "strings":
        assert (tree.distances == 0).sum() >= 74 and len(np.unique(tree.distances)) <= 7   # (at most 126 distinct strings among 200)
    assert ann.mst_rounds <= (ann.nx - 1).bit_length()      # (a round at least halves the components)


@pytest.mark.parametrize("cap", [None, 7])
def test_component_without_an_outside_anchor(cap):
    """All three anchors lie in cluster 0: once it is one component no anchor is outside it and it takes the cyclic bridge.  A
    tiny max_chunk_pairs spreads every round over several ranges and bisects rows."""
    from annchor_amd.pickers import SelectedAnchorPicker

    ann, want = _ann("clusters", n_anchors=3, anchor_picker=SelectedAnchorPicker([0, 1, 2]))
    tree = ann.minimum_spanning_tree(max_chunk_pairs=cap)
    assert M.same_tree(tree, want)
    assert tree.distances[-2] > 30 and ann.mst_rounds >= 2    # (a long edge is a component's lightest only once it is a whole cluster)
    # (every round has candidates -- its bridges pass their own bounds -- and 150 points are one range without a cap)
    assert ann.mst_chunks == ann.mst_rounds if cap is None else ann.mst_chunks > ann.mst_rounds


def test_python_callable_metric_goes_through_fetch_and_edges():
    from annchor_amd import Annchor, BruteForce

    X, _, D, want = M.case("pts130")
    calls = {"pairs": 0}

    def lookup(f, Xq, IJ):   # the object's evaluator: answers from the host table and counts what it is asked
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        calls["pairs"] += len(IJ)
        return D[IJ[:, 0], IJ[:, 1]]

    def host_metric(a, b):   # (a Python callable, so no device metric is bound; the pairs go through get_exact_ijs)
        raise AssertionError("not called one by one")

    ann = Annchor(list(X), host_metric, get_exact_ijs=lookup, n_anchors=5, **CFG)
    ann.get_anchors()
    before = calls["pairs"]
    assert M.same_tree(ann.minimum_spanning_tree(max_chunk_pairs=300), want)
    assert calls["pairs"] - before == ann.mst_evals      # only the bridges and the candidates were asked for
    assert M.same_tree(BruteForce(list(X), host_metric, get_exact_ijs=lookup).minimum_spanning_tree(), want)


def test_a_wrong_seed_costs_evaluations_only():
    ann, want = _ann("pts130")
    nn = np.argsort(M.case("pts130")[2], axis=1)[:, :2]                  # the true nearest neighbours
    assert M.same_tree(ann.minimum_spanning_tree(seed_graph=nn), want)
    rng = np.random.default_rng(3)
    assert M.same_tree(ann.minimum_spanning_tree(seed_graph=rng.integers(-5, 136, size=(130, 2))), want)
    assert M.same_tree(ann.minimum_spanning_tree(seed_graph=(np.full((130, 1), 130), None)), want)   # every partner invalid
    unseeded = ann.mst_evals
    assert M.same_tree(ann.minimum_spanning_tree(), want) and ann.mst_evals == unseeded
    for bad in (nn[:100], nn.astype(np.float64), nn[:, :0]):
        with pytest.raises(ValueError, match="seed_graph must hold integer indices"):
            ann.minimum_spanning_tree(seed_graph=bad)


def test_a_fitted_object_seeds_the_tree_and_is_left_as_it_was():
    from annchor_amd import Annchor

    X, metric, _, want = M.case("bundled320")
    ann = Annchor(X, metric, n_anchors=8, n_neighbors=10, n_samples=700, p_work=0.3, random_seed=42, niters=2).fit()
    ng0, graph0 = tuple(a.copy() for a in ann.neighbor_graph), ann._engine.neighbor_graph(10)
    q0 = ann.query(list(X[3:40:4]), nn=5)
    evals0 = ann.evals
    assert M.same_tree(ann.minimum_spanning_tree(), want) and ann.evals == evals0 + ann.mst_evals      # (no second anchor round)
    graph1 = ann._engine.neighbor_graph(10)
    assert all(np.array_equal(a, b) for a, b in zip(ng0, ann.neighbor_graph)) and all(np.array_equal(a, b) for a, b in zip(graph0, graph1))
    q1 = ann.query(list(X[3:40:4]), nn=5)
    assert np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])


def test_refusals():
    from annchor_amd import Annchor

    X = M.case("pts130")[0]
    ann = Annchor(X, "euclidean", n_anchors=5, **CFG)
    with pytest.raises(ValueError, match="bound_rtol must be in"):
        ann.minimum_spanning_tree(bound_rtol=1.0)
    with pytest.raises(ValueError, match="max_chunk_pairs must be >= 1"):
        ann.minimum_spanning_tree(max_chunk_pairs=0)
    with pytest.raises(ValueError, match=r"is_metric=False.*BruteForce\(X, func\)\.minimum_spanning_tree\(\)"):
        Annchor(X, "euclidean", n_anchors=5, is_metric=False, **CFG).minimum_spanning_tree()
    with pytest.raises(ValueError, match=r"cosine.*not a metric.*BruteForce\(X, 'cosine'\)\.minimum_spanning_tree\(\)"):
        Annchor(X + 5.0, "cosine", n_anchors=5, **CFG).minimum_spanning_tree()
    big = np.random.default_rng(0).standard_normal((2048, 16)).astype(np.float32)
    with pytest.raises(NotImplementedError, match=r"streamed=False.*BruteForce\(X, func\)\.minimum_spanning_tree\(\)"):
        Annchor(big, "euclidean", streamed=True, n_anchors=8, n_neighbors=5).minimum_spanning_tree()


def test_linkage_heights_equal_scipy_single_linkage():
    from annchor_amd import BruteForce
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform

    X, metric, D, want = M.case("pts130")
    assert len(np.unique(D[np.triu_indices(130, 1)])) == 130 * 129 // 2        # tie-free
    tree = BruteForce(X, metric).minimum_spanning_tree()
    Z, S = tree.linkage(), linkage(squareform(D, checks=False), method="single")
    assert Z.shape == S.shape and np.array_equal(Z[:, 2], S[:, 2]) and np.array_equal(Z[:, 3], S[:, 3])
    assert np.array_equal(Z[:, :2], np.sort(S[:, :2], axis=1))
    sp = tree.to_sparse_matrix()
    assert sp.shape == (130, 130) and sp.nnz == 2 * 129 and tree.total_weight == float(want[1].sum())
