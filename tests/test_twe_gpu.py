"""Time warp edit distance on the device (csrc/seqdp.hip) against the host recurrence of elastic_cases.py.

Tolerance: none.  Every cell is the min of three sums of fixed operands, min is exact and the additions are commutative, so
every evaluation order gives the same bits; each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import elastic_cases as lc
import pool_cases as pc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()
NU, LAM = 0.37, 0.21   # the non-default parameters of the tests below


# --------------------------------------------------------------------------------------------------- 1. small lengths
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim, longest, nu, lam", [(1, 40, 0.001, 1.0), (2, 96, 0.001, 1.0), (3, 40, 0.001, 1.0), (4, 40, 0.001, 1.0),
                                                   (1, 40, NU, LAM), (2, 96, NU, LAM)])
def test_small_lengths(dim, longest, nu, lam, dtype):
    """One series of each length 1..longest, all ordered pairs: n < m, n > m, n = m, length 1 against everything, every strip and
    group boundary of the 4-pairs-per-wavefront shape; then the list without its last 3 pairs (a last wavefront with one pair
    in it)."""
    X = lc.one_of_each_length(range(1, longest + 1), dim, seed=40 + dim, dtype=dtype)
    IJ = lc.all_ordered_pairs(len(X))
    want = ref(("small", dim, nu, np.dtype(dtype).name), lambda: lc.twe_pairs_host(X, IJ, nu, lam))
    assert np.all(np.isfinite(want))
    eng = pc.bound("twe", X, nu=nu, lam=lam)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T)


# ------------------------------------------------------------------------------------------------ 2. boundary lengths
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", lc.DIMS)
def test_boundary_lengths(dim, shape, dtype):
    """The strip and group boundaries {R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape (R, G) at this dim, the limit
    (distances.twe_max_length) and the limit minus 1, on the shape of each capacity.  One float32 random walk per length: the
    float64 data set is the same values widened, so both share a reference."""
    limit = lc.twe_max_length(dim)
    Ls = lc.boundary_lengths(dim, limit)
    R, G = lc.instantiations(dim, limit)[shape]
    assert {7, 8, 9, 16, 127, 128, 129, 511, 512, 513, limit - 1, limit} <= set(Ls)
    assert {R - 1, R, R + 1, 2 * R, G * R - 1, G * R} <= set(Ls)
    X = lc.one_of_each_length(Ls, dim, seed=50 + dim, dtype=np.float32)
    nkeep, IJ = lc.boundary_case(dim, limit, shape)
    sub = X[:nkeep]
    want = ref(("boundary", dim, shape), lambda: lc.twe_pairs_host(sub, IJ, NU, LAM))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("twe", [x.astype(dtype) for x in sub], IJ, nu=NU, lam=LAM)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- 3. coincident points
@pytest.mark.parametrize("dim", lc.DIMS)
def test_coincident_points(dim):
    """About a third of the points repeat their predecessor (dist = 0 and dx = nl there), and two members are constant: lengths
    1..70 crossed (the 4-pairs shape) and, in a second data set, a few lengths up to 300 (one pair per wavefront)."""
    for tag, lengths in (("short", range(1, 71)), ("long", [1, 2, 9, 64, 129, 200, 300])):
        X = lc.with_repeats(lc.one_of_each_length(lengths, dim, seed=70 + dim), seed=dim)
        X[3] = np.repeat(X[3][:1], len(X[3]), axis=0)
        X[5] = np.zeros_like(X[5])
        IJ = lc.all_ordered_pairs(len(X))
        want = ref(("repeats", dim, tag), lambda: lc.twe_pairs_host(X, IJ, NU, LAM))
        got = pc.device_pairs("twe", X, IJ, nu=NU, lam=LAM)
        assert np.array_equal(got, want)


# ----------------------------------------------------------------------------------------------- 4. PairSource forms
def fit_ref():
    """Every pair of the fit data set, [nx * nx]."""
    return ref("fit", lambda: pc.sym_matrix(lc.twe_pairs_host, lc.twe_fit_series()).ravel())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_ref()[IJ[:, 0] * len(lc.twe_fit_series()) + IJ[:, 1]])


def test_pair_source_forms():
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: ann.D), and positions into the pair list with the
    result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = lc.twe_fit_series()
    X[7] = X[3].copy()              # identical series
    nx = len(X)
    IJ = lc.all_ordered_pairs(nx)[::7]
    want = lc.twe_pairs_host(X, IJ)
    eng = pc.bound("twe", X)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, want)
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], lc.twe_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, "twe", **lc.FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], lc.twe_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], lc.twe_pairs_host(X, ann.IJs[done]))


@pytest.mark.parametrize("nu, lam", [(NU, LAM), (0.0, 0.5)])
def test_parameters_reach_the_kernel(nu, lam):
    """A second engine with other nu and lam on a univariate set, through explicit pairs, one-to-all and a fit: the values differ
    from the defaults', and equal the host's; nu = 0 is one case."""
    from annchor_amd import Annchor, _native

    X = lc.twe_univariate_series()
    nx = len(X)
    IJ = lc.all_ordered_pairs(nx)[::5]
    want = lc.twe_pairs_host(X, IJ, nu, lam)
    want0 = ref("defaults", lambda: lc.twe_pairs_host(X, IJ))
    assert not np.array_equal(want, want0)
    eng0, eng = pc.bound("twe", X), pc.bound("twe", X, nu=nu, lam=lam)
    got0, got = eng0.metric_pairs(IJ), eng.metric_pairs(IJ)
    eng.pick_anchors_selected([11])
    D = eng.download(_native.F_D).reshape(nx)
    eng0.close()
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got0, want0)
    assert np.array_equal(D, lc.twe_pairs_host(X, np.stack([np.full(nx, 11), np.arange(nx)], 1), nu, lam))
    ann = Annchor(X, "twe", func_kwargs={"nu": nu, "lam": lam}, **lc.FIT_CFG).fit()
    idx, dist = ann.neighbor_graph
    NN = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), lc.twe_pairs_host(X, NN, nu, lam))


# ------------------------------------------------------------------------------------------------------ 5. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = lc.twe_brute_series()
    assert len(X) == 200 and all(x.shape[1] == 3 for x in X) and len({len(x) for x in X}) > 20
    bf = BruteForce(X, "twe").fit()
    nx = len(X)
    T = pc.sym_matrix(lc.twe_pairs_host, X)
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 6. fits
def test_fit_parity_with_the_cpu_pipeline(capsys):
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = lc.twe_fit_series()
    nx = len(X)
    T = fit_ref().reshape(nx, nx)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)   # no ties within a row: the index comparisons rest on no tie rule
    ann = Annchor(X, "twe", ols="lapack", **lc.FIT_CFG).fit()
    ora = O.OracleAnnchor(nx, fit_pairs, **lc.FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    # the default solver: whatever the graph lists is an exact distance
    dflt = Annchor(X, "twe", **lc.FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(fit_pairs, nx)
    k = lc.FIT_CFG["n_neighbors"]
    print("twe is_metric=True, p_work=0.3: %d evaluations, %d of %d neighbours differ from the exact graph"
          % (dflt.evals, compare_neighbor_graphs(exact[:2], dflt.neighbor_graph, k), nx * k))


# ----------------------------------------------------------------------------------------------------------- 7. query
def test_query_with_other_lengths():
    """X is the fit data (240 series of dim 2, 20..60 points), Q a list of 20 series of 30..70 points."""
    from annchor_amd import Annchor

    X = lc.twe_fit_series()
    Q = lc.clustered_curves(20, 30, 70, 2, seed=49)
    assert len(X) == 240 and min(map(len, Q)) >= 30 and max(map(len, Q)) <= 70 and len({len(q) for q in Q}) > 5
    both = list(X) + Q
    nx = len(X)
    ann = Annchor(X, "twe", ols="lapack", **lc.FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, lambda IJ: lc.twe_pairs_host(both, IJ), **lc.FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: lc.twe_pairs_host(both, np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5,
                           p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# --------------------------------------------------------------------------------------------------- 8. loose objects
def test_loose_objects():
    from annchor_amd.distances import TWE, twe

    rng = np.random.default_rng(6)
    xs = [np.cumsum(rng.standard_normal((L, 3)), axis=0) for L in (5, 40, 1, 130)]
    ys = [np.cumsum(rng.standard_normal((L, 3)), axis=0) for L in (17, 9, 33, 2)]
    assert twe(xs[0], ys[0]) == lc.twe_loop(xs[0], ys[0])
    assert twe(ys[1], xs[1]) == lc.twe_loop(ys[1], xs[1])
    assert np.array_equal(twe.many(xs, ys), [lc.twe_loop(x, y) for x, y in zip(xs, ys)])
    assert np.array_equal(twe.one_to_many(xs[1], ys), [lc.twe_loop(xs[1], y) for y in ys])
    # univariate members
    a, b = rng.standard_normal(12), rng.standard_normal(7)
    assert twe(a, b) == lc.twe_loop(a, b)
    # the known answers
    for x, y, nu, lam, want in (([1, 2, 3], [2, 2, 2], 0.25, 0.5, 3.0), ([0], [4], 0.5, 1.0, 4.0),
                                ([1, 1, 1, 5], [1, 5], 0.125, 0.5, 1.75), ([3, 1, 4, 1, 5], [2, 7, 1], 0.5, 1.0, 19.0)):
        assert TWE(nu=nu, lam=lam)(np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)) == want
        assert TWE(nu=nu, lam=lam)(np.array(y, dtype=np.float32), np.array(x, dtype=np.float32)) == want
    # parameters of its own
    t2 = TWE(nu=NU, lam=LAM)
    assert t2(a, b) == lc.twe_loop(a, b, NU, LAM) != twe(a, b)
    assert np.array_equal(t2.many(xs, ys), [lc.twe_loop(x, y, NU, LAM) for x, y in zip(xs, ys)])


# ---------------------------------------------------------------------------------------------------------- 9. limits
def test_limits():
    from annchor_amd import BruteForce, _native
    from annchor_amd.distances import TWE

    rng = np.random.default_rng(5)
    L1, L2 = lc.twe_max_length(1), lc.twe_max_length(2)
    with pytest.raises(ValueError, match="twe: series 0 has %d points" % (L1 + 1)):
        BruteForce([rng.standard_normal(L1 + 1), rng.standard_normal(10)], "twe")
    with pytest.raises(ValueError, match="twe: series 1 has %d points" % (L2 + 1)):
        BruteForce([rng.standard_normal((10, 2)), rng.standard_normal((L2 + 1, 2))], "twe")
    with pytest.raises(ValueError, match="twe: series 0 has dim 5"):
        BruteForce([rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], "twe")
    with pytest.raises(ValueError, match="twe: series 1 has dim 3, series 0 has dim 2"):
        BruteForce([rng.standard_normal((10, 2)), rng.standard_normal((10, 3))], "twe")
    with pytest.raises(ValueError, match="twe: series 1 is empty"):
        BruteForce([rng.standard_normal((10, 2)), np.zeros((0, 2))], "twe")
    with pytest.raises(ValueError, match="twe: series 0 .*not finite"):
        BruteForce([np.array([1.0, np.nan]), rng.standard_normal(10)], "twe")
    with pytest.raises(ValueError, match="twe: nu must be a finite real number >= 0"):
        TWE(nu=-1.0)
    with pytest.raises(ValueError, match="twe: lam must be a finite real number >= 0"):
        BruteForce([rng.standard_normal(10), rng.standard_normal(10)], "twe", func_kwargs={"lam": np.nan})
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        v1 = rng.standard_normal(L1 + 1 + 10)
        with pytest.raises(_native.NativeError, match=r"error -4: .*%d.*1\.\.%d at dim 1" % (L1 + 1, L1)):
            eng.set_twe_series(v1, np.array([0, L1 + 1]), np.array([L1 + 1, 10]), 1)
        v = rng.standard_normal((L2 + 1 + 10) * 2)
        with pytest.raises(_native.NativeError, match=r"error -4: .*%d.*1\.\.%d at dim 2" % (L2 + 1, L2)):
            eng.set_twe_series(v, np.array([0, L2 + 1]), np.array([L2 + 1, 10]), 2)
        with pytest.raises(_native.NativeError, match=r"error -4: .*dim 5"):
            eng.set_twe_series(v, np.array([0, 10]), np.array([10, 10]), 5)
        with pytest.raises(_native.NativeError, match=r"error -1: .*empty"):
            eng.set_twe_series(v, np.array([0, 10]), np.array([10, 0]), 2)
        for bad in (np.nan, np.inf, -0.5):
            with pytest.raises(_native.NativeError, match=r"error -1: twe: the stiffness nu"):
                eng.set_twe_series(v, np.array([0, 10]), np.array([10, 10]), 2, bad, 1.0)
            with pytest.raises(_native.NativeError, match=r"error -1: twe: the penalty lam"):
                eng.set_twe_series(v, np.array([0, 10]), np.array([10, 10]), 2, 0.001, bad)
        v[3] = np.nan
        with pytest.raises(_native.NativeError, match="error -1: .*non-finite"):
            eng.set_twe_series(v, np.array([0, L2]), np.array([L2, 10]), 2)
    finally:
        eng.close()
