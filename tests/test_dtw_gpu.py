"""DTW on the device (csrc/seqdp.hip) against the host recurrence of dtw_cases.py.

Tolerance: none.  min is exact and every cell of the recurrence has fixed operands, so every evaluation order gives the same
bits; each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import dtw_cases as dc
import pool_cases as pc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()


# --------------------------------------------------------------------------------------------------- 1. small lengths
def small_series(dtype):
    return dc.one_of_each_length(range(1, 97), seed=21, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("window", [None, 0, 5])
def test_small_lengths(window, dtype):
    """One series of each length 1..96, all 9216 ordered pairs: n < m, n > m, n = m, every strip and group boundary of the
    4-pairs-per-wavefront instantiation; then the list without its last 3 pairs (a last wavefront with one pair in it)."""
    X = small_series(dtype)
    IJ = dc.all_ordered_pairs(len(X))
    want = ref(("small", np.dtype(dtype).name, window), lambda: dc.dtw_pairs_host(X, IJ, window))
    assert np.all(np.isfinite(want))
    eng = pc.bound("dtw", X, window=window)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


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
    return ref(("large", window), lambda: dc.dtw_pairs_host(X, dc.all_ordered_pairs(len(X)), window))


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


# ----------------------------------------------------------------------------------------------- 3. PairSource forms
def fit_ref():
    """Every pair of the fit data set, [nx * nx]."""
    return ref("fit", lambda: pc.sym_matrix(dc.dtw_pairs_host, dc.fit_series()).ravel())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_ref()[IJ[:, 0] * len(dc.fit_series()) + IJ[:, 1]])


def test_pair_source_forms():
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: ann.D), and positions into the pair list with the
    result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = dc.fit_series()
    X[7] = X[3].copy()              # identical series
    nx = len(X)
    IJ = dc.all_ordered_pairs(nx)[::7]
    want = dc.dtw_pairs_host(X, IJ, None)
    eng = pc.bound("dtw", X)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, want)
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], dc.dtw_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1), None))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, "dtw", is_metric=False, **dc.FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], dc.dtw_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1), None))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], dc.dtw_pairs_host(X, ann.IJs[done], None))


# ------------------------------------------------------------------------------------------------------ 4. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = dc.brute_series()
    assert len(X) == 200 and len({len(x) for x in X}) > 20
    bf = BruteForce(X, "dtw").fit()
    oi, od, _ = O.brute_force(lambda IJ: dc.dtw_pairs_host(X, IJ, None), len(X))
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# -------------------------------------------------------------------------------------------------------- 5, 6. fits
def test_fit_parity_with_the_cpu_pipeline(capsys):
    from annchor_amd import Annchor

    X = dc.fit_series()
    ann = Annchor(X, "dtw", ols="lapack", **dc.FIT_CFG)
    assert "triangle inequality" in capsys.readouterr().err
    ann.fit()
    ora = O.OracleAnnchor(len(X), fit_pairs, **dc.FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])


def test_fit_without_the_triangle_inequality(capsys):
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = dc.fit_series()
    nx = len(X)

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


# ----------------------------------------------------------------------------------------------------------- 7. query
def test_query_with_other_lengths():
    """X is an array (rows of 48 values), Q a list of 20 series of 30..70 values."""
    from annchor_amd import Annchor

    X = np.stack(dc.clustered_series(240, 48, 48, seed=13))
    Q = dc.clustered_series(20, 30, 70, seed=14)
    assert X.shape == (240, 48) and min(map(len, Q)) >= 30 and max(map(len, Q)) <= 70 and len({len(q) for q in Q}) > 5
    both = list(X) + Q
    nx = len(X)
    ann = Annchor(X, "dtw", ols="lapack", **dc.FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, lambda IJ: dc.dtw_pairs_host(both, IJ, None), **dc.FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: dc.dtw_pairs_host(both, np.stack([IJ[:, 0], IJ[:, 1] + nx], 1), None), len(Q), nn=5,
                           p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# ---------------------------------------------------------------------------------------------------------- 8. limits
def test_limits():
    from annchor_amd import BruteForce, _native

    rng = np.random.default_rng(5)
    with pytest.raises(ValueError, match="2049"):
        BruteForce([rng.standard_normal(2049), rng.standard_normal(10)], "dtw")
    with pytest.raises(_native.NativeError, match="error -4"):
        BruteForce([rng.standard_normal(10)], "dtw")
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        v = rng.standard_normal(2049 + 10)
        with pytest.raises(_native.NativeError, match=r"error -4: .*2049.*1\.\.2048"):
            eng.set_series(v, np.array([0, 2049]), np.array([2049, 10]))
        v[3] = np.nan
        with pytest.raises(_native.NativeError, match="error -1: .*non-finite"):
            eng.set_series(v, np.array([0, 2048]), np.array([2048, 10]))
    finally:
        eng.close()
