"""The discrete Frechet distance on the device (csrc/seqdp.hip) against the host recurrence of frechet_cases.py.

Tolerance: none.  max and min are exact and every c(i, j) has fixed operands, so every evaluation order gives the same bits;
each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import frechet_cases as fc
import pool_cases as pc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()


# --------------------------------------------------------------------------------------------------- 1. small lengths
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim, longest", [(2, 96), (1, 40), (3, 40), (4, 40)])
def test_small_lengths(dim, longest, dtype):
    """One curve of each length 1..longest, all ordered pairs: n < m, n > m, n = m, every strip and group boundary of the
    4-pairs-per-wavefront shape; then the list without its last 3 pairs (a last wavefront with one pair in it)."""
    X = fc.one_of_each_length(range(1, longest + 1), dim, seed=40 + dim, dtype=dtype)
    IJ = fc.all_ordered_pairs(len(X))
    want = ref(("small", dim, np.dtype(dtype).name), lambda: fc.frechet_pairs_host(X, IJ))
    assert np.all(np.isfinite(want))
    eng = pc.bound("frechet", X)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


# ------------------------------------------------------------------------------------------------ 2. boundary lengths
def boundary_curves(dim):
    """One float32 random walk per boundary length: the float64 data set is the same values widened, so both share a reference."""
    return fc.one_of_each_length(fc.boundary_lengths(dim), dim, seed=50 + dim, dtype=np.float32)


def boundary_case(dim, shape):
    """The data set that runs shape number `shape` at `dim` -- the kernel is chosen by the data set's longest curve, so it holds
    the boundary lengths up to the shape's capacity R G -- and its pair list.  Up to 512 points all lengths are crossed; at the
    widest shape each length meets {1, R, the limit} in both orders (a rectangle: the full crossing's host reference is slow)."""
    Ls = fc.boundary_lengths(dim)
    R, G = fc.instantiations(dim)[shape]
    cap = R * G
    nkeep = sum(L <= cap for L in Ls)   # (Ls ascends: the data set is its first nkeep curves)
    assert Ls[nkeep - 1] == cap
    if cap <= 512:
        IJ = fc.all_ordered_pairs(nkeep)
    else:
        assert cap == fc.max_length(dim)
        partners = [Ls.index(L) for L in (1, R, cap)]
        IJ = np.array([p for k in range(nkeep) for q in partners for p in ((k, q), (q, k))], dtype=np.int64)
    return nkeep, IJ


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", fc.DIMS)
def test_boundary_lengths(dim, shape, dtype):
    """The strip and group boundaries {R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape (R, G) at this dim, the limit and the limit
    minus 1, on the shape of each capacity."""
    Ls, X = fc.boundary_lengths(dim), boundary_curves(dim)
    R, G = fc.instantiations(dim)[shape]
    assert {7, 8, 9, 16, 127, 128, 129, 511, 512, 513, fc.max_length(dim) - 1, fc.max_length(dim)} <= set(Ls)
    assert {R - 1, R, R + 1, 2 * R, G * R - 1, G * R} <= set(Ls)
    nkeep, IJ = boundary_case(dim, shape)
    sub = X[:nkeep]
    want = ref(("boundary", dim, shape), lambda: fc.frechet_pairs_host(sub, IJ))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("frechet", [x.astype(dtype) for x in sub], IJ)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------------------------- 3. PairSource forms
def fit_ref():
    """Every pair of the fit data set, [nx * nx]."""
    return ref("fit", lambda: pc.sym_matrix(fc.frechet_pairs_host, fc.fit_curves()).ravel())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_ref()[IJ[:, 0] * len(fc.fit_curves()) + IJ[:, 1]])


def test_pair_source_forms():
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: ann.D), and positions into the pair list with the
    result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = fc.fit_curves()
    X[7] = X[3].copy()              # identical curves
    nx = len(X)
    IJ = fc.all_ordered_pairs(nx)[::7]
    want = fc.frechet_pairs_host(X, IJ)
    eng = pc.bound("frechet", X)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, want)
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], fc.frechet_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, "frechet", **fc.FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], fc.frechet_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], fc.frechet_pairs_host(X, ann.IJs[done]))


# ------------------------------------------------------------------------------------------------------ 4. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = fc.brute_curves()
    assert len(X) == 200 and all(x.shape[1] == 3 for x in X) and len({len(x) for x in X}) > 20
    bf = BruteForce(X, "frechet").fit()
    nx = len(X)
    T = pc.sym_matrix(fc.frechet_pairs_host, X)
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 5. fits
def test_fit_parity_with_the_cpu_pipeline(capsys):
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = fc.fit_curves()
    nx = len(X)
    ann = Annchor(X, "frechet", ols="lapack", **fc.FIT_CFG).fit()
    ora = O.OracleAnnchor(nx, fit_pairs, **fc.FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    # the default solver: whatever the graph lists is an exact distance
    dflt = Annchor(X, "frechet", **fc.FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(fit_pairs, nx)
    k = fc.FIT_CFG["n_neighbors"]
    print("is_metric=True, p_work=0.3: %d of %d neighbours differ from the exact graph"
          % (compare_neighbor_graphs(exact[:2], dflt.neighbor_graph, k), nx * k))


# ----------------------------------------------------------------------------------------------------------- 6. query
def test_query_with_other_lengths():
    """X is a 3-D array [240, 48, 2], Q a list of 20 curves of 30..70 points."""
    from annchor_amd import Annchor

    X = np.stack(fc.clustered_curves(240, 48, 48, 2, seed=33))
    Q = fc.clustered_curves(20, 30, 70, 2, seed=34)
    assert X.shape == (240, 48, 2) and min(map(len, Q)) >= 30 and max(map(len, Q)) <= 70 and len({len(q) for q in Q}) > 5
    both = list(X) + Q
    nx = len(X)
    ann = Annchor(X, "frechet", ols="lapack", **fc.FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, lambda IJ: fc.frechet_pairs_host(both, IJ), **fc.FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: fc.frechet_pairs_host(both, np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5,
                           p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# --------------------------------------------------------------------------------------------------- 7. loose objects
def test_loose_objects():
    from annchor_amd.distances import frechet

    rng = np.random.default_rng(6)
    xs = [np.cumsum(rng.standard_normal((L, 3)), axis=0) for L in (5, 40, 1, 130)]
    ys = [np.cumsum(rng.standard_normal((L, 3)), axis=0) for L in (17, 9, 33, 2)]
    assert frechet(xs[0], ys[0]) == fc.frechet_loop(xs[0], ys[0])
    assert frechet(ys[1], xs[1]) == fc.frechet_loop(ys[1], xs[1])
    assert np.array_equal(frechet.many(xs, ys), [fc.frechet_loop(x, y) for x, y in zip(xs, ys)])
    assert np.array_equal(frechet.one_to_many(xs[1], ys), [fc.frechet_loop(xs[1], y) for y in ys])
    # univariate members
    a, b = rng.standard_normal(12), rng.standard_normal(7)
    assert frechet(a, b) == fc.frechet_loop(a, b)


# ---------------------------------------------------------------------------------------------------------- 8. limits
def test_limits():
    from annchor_amd import BruteForce, _native

    rng = np.random.default_rng(5)
    with pytest.raises(ValueError, match="curve 0 has 2049 points"):
        BruteForce([rng.standard_normal((2049, 2)), rng.standard_normal((10, 2))], "frechet")
    with pytest.raises(ValueError, match="curve 1 has 1025 points"):
        BruteForce([rng.standard_normal((10, 3)), rng.standard_normal((1025, 3))], "frechet")
    with pytest.raises(ValueError, match="curve 0 has dim 5"):
        BruteForce([rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], "frechet")
    with pytest.raises(ValueError, match="curve 1 has dim 3, curve 0 has dim 2"):
        BruteForce([rng.standard_normal((10, 2)), rng.standard_normal((10, 3))], "frechet")
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        v = rng.standard_normal((2049 + 10) * 2)
        with pytest.raises(_native.NativeError, match=r"error -4: .*2049.*1\.\.2048"):
            eng.set_curves(v, np.array([0, 2049]), np.array([2049, 10]), 2)
        v3 = rng.standard_normal((1025 + 10) * 3)
        with pytest.raises(_native.NativeError, match=r"error -4: .*1025.*1\.\.1024"):
            eng.set_curves(v3, np.array([0, 1025]), np.array([1025, 10]), 3)
        with pytest.raises(_native.NativeError, match=r"error -4: .*dim 5"):
            eng.set_curves(v, np.array([0, 10]), np.array([10, 10]), 5)
        with pytest.raises(_native.NativeError, match=r"error -1: .*empty"):
            eng.set_curves(v, np.array([0, 10]), np.array([10, 0]), 2)
        v[3] = np.nan
        with pytest.raises(_native.NativeError, match="error -1: .*non-finite"):
            eng.set_curves(v, np.array([0, 2048]), np.array([2048, 10]), 2)
    finally:
        eng.close()
