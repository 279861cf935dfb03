"""DTW on the device (csrc/seqdp.hip): the tests it alone has, and its cases of the small-length section; the other sections are
test_seqdp_gpu.py's.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import dtw_cases as dc
import pool_cases as pc
import test_seqdp_gpu as suite
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

S = suite.BY_NAME["dtw"]


# --------------------------------------------------------------------------------------------------- 1. small lengths
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("window", [None, 0, 5])
def test_small_lengths(window, dtype):
    """One series of each length 1..96, all 9216 ordered pairs."""
    X = dc.one_of_each_length(range(1, 97), seed=21, dtype=dtype)
    suite.small_lengths(S, X, (window, np.dtype(dtype).name), window=window)


# --------------------------------------------------------------------------------------------------- 2. large lengths
def large_lengths():
    Ls = {127, 128, 129, 1023, 1024, 1025, 2047, 2048}
    for R, G in dc.INSTANTIATIONS:
        Ls.update(dc.boundary_lengths(R, G))
    return sorted(Ls)


def large_series():
    return dc.one_of_each_length(large_lengths(), seed=22)


def large_ref(window):
    X = large_series()
    return suite.ref(("dtw", "large", window), lambda: dc.dtw_pairs_host(X, dc.all_ordered_pairs(len(X)), window))


@pytest.mark.parametrize("window", [None, 64])
@pytest.mark.parametrize("cap", [128, 512, 2048])
def test_large_lengths(cap, window):
    """The strip and group boundaries of every instantiation ({R-1, R, R+1, 2R, GR-1, GR, GR+1} for (R, G) = (8, 16), (8, 64),
    (32, 64)) plus 127..129, 1023..1025, 2047, 2048, all crossed.  The kernel is chosen by the data set's longest series, so the
    lengths up to `cap` form the data set that runs the instantiation of that capacity; cap = 2048 holds all of them.
    window = 64 is narrower than |n - m| for most pairs (the band then reaches the corner) and wider for the rest."""
    Ls, X = large_lengths(), large_series()
    assert {7, 8, 9, 16, 127, 128, 129, 511, 512, 513, 31, 32, 33, 64, 2047, 2048} <= set(Ls)
    keep = np.array([k for k, L in enumerate(Ls) if L <= cap])
    assert Ls[keep[-1]] == cap
    nall = len(Ls)
    sub = dc.all_ordered_pairs(len(keep))
    want = large_ref(window)[keep[sub[:, 0]] * nall + keep[sub[:, 1]]]
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("dtw", [X[k] for k in keep], sub, window=window)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("window", [0, 64])
@pytest.mark.parametrize("shape, lengths", [((8, 64), (1, 129, 511, 512)), ((32, 64), (1, 513, 2047, 2048))])
def test_banded_float32_wide_shapes(shape, lengths, window):
    """The banded kernel on float32 input at the two one-pair-per-wavefront shapes (test_large_lengths is float64, the banded
    float32 cases of test_small_lengths run (8, 16)): the shortest series, the first length past the narrower shape and the
    shape's last two lengths, all 16 ordered pairs."""
    R, G = shape
    assert shape in dc.INSTANTIATIONS and max(lengths) == R * G   # (the longest series of the data set selects the shape)
    X = dc.one_of_each_length(lengths, seed=23, dtype=np.float32)
    assert all(x.dtype == np.float32 for x in X)
    IJ = dc.all_ordered_pairs(len(X))
    want = dc.dtw_pairs_host(X, IJ, window)
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("dtw", X, IJ, window=window)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------- 3. the fit that is told it is no metric
def test_fit_without_the_triangle_inequality(capsys):
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = dc.fit_series()
    nx = len(X)
    fit_pairs = suite.fit_pairs(S)

    def evaluator(f, Xs, IJ):
        return fit_pairs(IJ)

    dev = Annchor(X, "dtw", is_metric=False, ols="lapack", **dc.FIT_CFG)
    assert "triangle inequality" not in capsys.readouterr().err
    dev.fit()
    host = Annchor(X, "dtw", is_metric=False, ols="lapack", get_exact_ijs=evaluator, **dc.FIT_CFG).fit()
    assert dev.evals == host.evals
    assert np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1])
    assert np.array_equal(dev.neighbor_graph[0], host.neighbor_graph[0])
    # the default solver: whatever the graph lists is an exact distance
    ann = Annchor(X, "dtw", is_metric=False, **dc.FIT_CFG).fit()
    idx, dist = ann.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(fit_pairs, nx)
    k = dc.FIT_CFG["n_neighbors"]
    print("is_metric=False, p_work=0.3: %d of %d neighbours differ from the exact graph"
          % (compare_neighbor_graphs(exact[:2], ann.neighbor_graph, k), nx * k))
