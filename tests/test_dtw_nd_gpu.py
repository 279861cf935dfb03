"""DTW on series of 2 .. 4 coordinates per point on the device (csrc/seqdp.hip, DtwOp at DIM > 1) against the host sweep of
seqdp_cases.py.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import frechet_cases as fc
import pool_cases as pc
import seqdp_cases as sc
import test_seqdp_gpu as suite
import threshold_cases as tc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
S = suite.spec("dtw", sc.dtw_pairs_host)
DIMS = [2, 3, 4]
WINDOWS = [None, 0, 64]


def boundary_data(dim):
    return sc.one_of_each_length(sc.boundary_lengths("dtw", dim), dim, seed=60 + dim, dtype=F32)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("window", [None, 0, 5])
def test_small_lengths(window, dtype):
    """One series of dim 3 of each length 1..96, all 9216 ordered pairs."""
    X = sc.one_of_each_length(range(1, 97), 3, seed=24, dtype=dtype)
    suite.small_lengths(S, X, ("nd", window, np.dtype(dtype).name), window=window)


@pytest.mark.parametrize("shape, dtype", [(0, F64), (0, F32), (1, F64), (2, F64), (2, F32)])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("dim", DIMS)
def test_boundary_lengths(dim, window, shape, dtype):
    """seqdp_cases.boundary_case at every shape; window = 64 is narrower than |n - m| for most pairs and wider for the rest."""
    R, G = sc.instantiations("dtw", dim)[shape]
    nkeep, IJ = sc.boundary_case("dtw", dim, shape)
    sub = boundary_data(dim)[:nkeep]
    assert max(map(len, sub)) == R * G
    want = suite.ref(("dtw", "nd-boundary", dim, shape, window), lambda: sc.dtw_pairs_host(sub, IJ, window))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("dtw", [x.astype(dtype) for x in sub], IJ, window=window)
    assert np.array_equal(got, want)


def test_univariate_members_through_both_entry_points():
    """[len, 1] members go through set_series_nd at dim 1, [len] members through set_series: the same bits."""
    X = sc.one_of_each_length([1, 7, 64, 130, 600], 1, seed=25)
    IJ = pc.all_ordered_pairs(len(X))
    for window in (None, 3):
        want = sc.dtw_pairs_host(X, IJ, window)
        assert np.array_equal(pc.device_pairs("dtw", X, IJ, window=window), want)
        assert np.array_equal(pc.device_pairs("dtw", sc.univariate(X), IJ, window=window), want)


def test_loose_objects():
    from annchor_amd import distances

    rng = np.random.default_rng(6)
    x, y = np.cumsum(rng.standard_normal((40, 3)), axis=0), np.cumsum(rng.standard_normal((17, 3)), axis=0)
    assert distances.DTW()(x, y) == tc.dtw_loop(x, y) == distances.dtw(y, x)
    assert distances.DTW(window=2)(x, y) == tc.dtw_loop(x, y, 2)
    assert np.array_equal(distances.dtw.many([x, y], [y, y]), [tc.dtw_loop(x, y), 0.0])


def test_limits():
    from annchor_amd import _native

    rng = np.random.default_rng(5)
    for match, X in [("dtw: series 0 has 2049 points; at most 2048 are supported at dim 2", [rng.standard_normal((2049, 2)), rng.standard_normal((10, 2))]),
                     ("dtw: series 1 has 1025 points", [rng.standard_normal((10, 3)), rng.standard_normal((1025, 3))]),
                     ("dtw: series 0 has dim 5", [rng.standard_normal((10, 5)), rng.standard_normal((10, 5))]),
                     ("dtw: series 1 has dim 3, series 0 has dim 2", [rng.standard_normal((10, 2)), rng.standard_normal((10, 3))]),
                     ("dtw: series 1 is empty", [rng.standard_normal((10, 2)), np.zeros((0, 2))]),
                     ("dtw: series 0 .*not finite", [np.full((3, 2), np.nan), rng.standard_normal((10, 2))])]:
        suite.raises_value_error(match, X, "dtw")
    v3 = rng.standard_normal((1025 + 10) * 3)
    bad = v3.copy()
    bad[3] = np.nan
    eng = _native.Engine(0)
    try:
        for match, args in [(r"error -4: .*1025.*1\.\.1024 at dim 3", (v3, [0, 1025], [1025, 10], 3)),
                            (r"error -4: .*dim 5", (v3, [0, 10], [10, 10], 5)),
                            (r"error -1: .*empty", (v3, [0, 10], [10, 0], 3)),
                            ("error -1: .*non-finite", (bad, [0, 1024], [1024, 10], 3))]:
            with pytest.raises(_native.NativeError, match=match):
                eng.set_series_nd(args[0], np.array(args[1]), np.array(args[2]), args[3])
        w = rng.standard_normal((1024 + 10, 3))
        eng.set_series_nd(w.ravel(), np.array([0, 1024]), np.array([1024, 10]), 3, window=7)
        assert eng.metric_pairs(np.array([[0, 1]]))[0] == sc.dtw_pairs_host([w[:1024], w[1024:]], [[0, 1]], 7)[0]
    finally:
        eng.close()


def test_fit_brute_force_and_query():
    from annchor_amd import Annchor, BruteForce

    X, Q = fc.fit_curves(), sc.clustered_curves(20, 30, 70, 2, seed=34)
    nx, nall = len(X), len(X) + len(Q)
    T = suite.ref(("dtw", "nd-fit"), lambda: pc.sym_matrix(sc.dtw_pairs_host, X + Q).ravel())

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(T[IJ[:, 0] * nall + IJ[:, 1]])

    def evaluator(f, Xs, IJ):
        return pairs(IJ)

    def query_evaluator(f, Xs, Z, IJ):
        """Pairs (Xs[i], Z[j]); Xs is the data set, or its anchors in the order of host.A."""
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        rows = IJ[:, 0] if len(Xs) == nx else np.asarray(host.A, dtype=np.int64)[IJ[:, 0]]
        return pairs(np.stack([rows, IJ[:, 1] + nx], axis=1))

    dev = Annchor(X, "dtw", is_metric=False, ols="lapack", **pc.FIT_CFG).fit()
    host = Annchor(X, "dtw", is_metric=False, ols="lapack", get_exact_ijs=evaluator, **pc.FIT_CFG).fit()
    assert dev.evals == host.evals
    assert np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1])
    assert np.array_equal(dev.neighbor_graph[0], host.neighbor_graph[0])
    bf = BruteForce(X, "dtw").fit()
    oi, od, _ = O.brute_force(pairs, nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)
    gi, gd = dev.query(Q, nn=5, p_work=0.3)
    hi, hd = host.query(Q, nn=5, p_work=0.3, get_exact_query_ijs=query_evaluator)
    assert dev.query_evals == host.query_evals
    assert np.array_equal(gd, hd)
    assert np.array_equal(gi, hi)
