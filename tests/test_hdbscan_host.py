"""The host extraction of HDBSCAN* alone (annchor_amd/radius.py: condense, select, hdbscan_labels) on trees that
mst_cases.kruskal builds from NumPy Euclidean mutual-reachability matrices: no GPU.  Three blobs of different density with
planted far outliers, continuous coordinates (no duplicate points, no two equal distances), against scikit-learn's
HDBSCAN(metric="precomputed") at its defaults: the same noise mask and a one-to-one map between the label sets.  Mutual-
reachability weights tie even on such data, and scikit-learn takes merges of equal height in another order than (w, i, j); on
this input the three parameter pairs give the same labels either way, and no input had to be replaced."""
import functools

import numpy as np
import pytest

import mst_cases as M
from annchor_amd import radius

OUTLIERS = np.array([[60.0, 60.0], [-50.0, 45.0], [55.0, -40.0], [-45.0, -55.0]])


@functools.lru_cache(maxsize=None)
def blobs():
    """(dense matrix, blob of every point): 40 + 30 + 25 points at scales 1, 0.5 and 2 around centres at least 25 apart, then
    the four outliers, each farther from every blob than any blob is wide."""
    rng = np.random.default_rng(11)
    parts = [rng.standard_normal((n, 2)) * s + c for n, s, c in ((40, 1.0, [0.0, 0.0]), (30, 0.5, [25.0, 0.0]), (25, 2.0, [0.0, 30.0]))]
    X = np.concatenate(parts + [OUTLIERS])
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    return D, np.repeat([0, 1, 2, -1], [40, 30, 25, len(OUTLIERS)])


def reach_tree(D, m):
    core = np.sort(D, axis=1)[:, m - 1]
    W = np.maximum(D, np.maximum(core[:, None], core[None, :]))
    return radius.SpanningTree(*M.kruskal(W), len(D), core, m)


@pytest.mark.parametrize("min_cluster_size,min_samples", [(5, 5), (8, 1), (10, 3)])
def test_labels_equal_scikit_learn(min_cluster_size, min_samples):
    cluster = pytest.importorskip("sklearn.cluster")
    D, _ = blobs()
    got, n = radius.hdbscan_labels(reach_tree(D, min_samples), min_cluster_size)
    want = cluster.HDBSCAN(metric="precomputed", min_cluster_size=min_cluster_size, min_samples=min_samples).fit(D.copy()).labels_
    assert np.array_equal(got < 0, want < 0)
    pairs = set(zip(got[got >= 0].tolist(), want[want >= 0].tolist()))
    assert len(pairs) == n == len(set(want[want >= 0].tolist()))          # one-to-one: as many pairs as labels on either side


def test_three_blobs_and_planted_outliers():
    D, blob = blobs()
    labels, n = radius.hdbscan_labels(reach_tree(D, 5), 5)
    assert n == 3 and np.array_equal(labels[blob < 0], [-1] * len(OUTLIERS))
    for b in range(3):      # a blob is one cluster (its sparse fringe may be noise), numbered by its smallest member
        inside = labels[blob == b]
        assert set(inside[inside >= 0].tolist()) == {b}


def test_coincident_points_are_one_cluster():
    """A hand-made dendrogram: two groups of six coincident points merge at height 0 (lambda = inf), each enough for a cluster of
    min_cluster_size 5, beside six points that merge at height 1.  The twelve stay one cluster, every birth is finite and no
    stability is inf - inf."""
    rows = []

    def chain(top, others, h):      # the points join one by one; returns the last merge's node
        for size, p in enumerate(others, 2):
            rows.append((min(top, p), max(top, p), h, size))
            top = 18 + len(rows) - 1
        return top

    a, b = chain(0, range(1, 6), 0.0), chain(6, range(7, 12), 0.0)
    rows.append((a, b, 0.0, 12))
    ab, c = 18 + len(rows) - 1, chain(12, range(13, 18), 1.0)
    rows.append((ab, c, 10.0, 18))
    with np.errstate(invalid="raise"):
        ct = radius.condense(np.array(rows), 5)
        own = radius.select(ct)[ct["point_cluster"]]
    assert len(ct["parent"]) == 3 and np.isfinite(ct["birth"]).all() and np.isinf(ct["point_lambda"][:12]).all()
    assert set(own[:12].tolist()) == {1} and set(own[12:].tolist()) == {2}


def test_argument_errors():
    for bad in (1, 0, 2.0, True):
        with pytest.raises(ValueError, match=r"min_cluster_size must be an integer >= 2"):
            radius.check_hdbscan(bad, None, 100)
    for bad in (0, 101, 2.5):
        with pytest.raises(ValueError, match=r"min_samples must be an integer in 1\.\.100"):
            radius.check_hdbscan(5, bad, 100)
    assert radius.check_hdbscan(7, None, 100) == (7, 7)
