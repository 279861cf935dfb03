"""The Hausdorff distance on the device (csrc/hausdorff.hip) against the host definition of hausdorff_cases.py.

Tolerance: none.  min and max are exact and every c(i, j) has fixed operands, so every evaluation order gives the same bits;
each comparison of distances below is np.array_equal."""
import numpy as np
import pytest

import hausdorff_cases as hc
import pool_cases as pc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()


# ----------------------------------------------------------------------------------------------------- 1. small sizes
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim, longest", [(2, 96), (1, 40), (3, 40), (4, 40)])
def test_small_sizes(dim, longest, dtype):
    """One set of each size 1..longest, all ordered pairs: n < m, n > m, n = m, four pairs of unequal sizes in a wavefront; then
    the list without its last 3 pairs (a last wavefront with one pair in it)."""
    X = hc.one_of_each_length(range(1, longest + 1), dim, seed=60 + dim, dtype=dtype)
    IJ = hc.all_ordered_pairs(len(X))
    want = ref(("small", dim, np.dtype(dtype).name), lambda: hc.hausdorff_pairs_host(X, IJ))
    assert np.all(np.isfinite(want))
    eng = pc.bound("hausdorff", X)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


# -------------------------------------------------------------------------------------------------- 2. boundary sizes
def boundary_sets(dim):
    """One float32 random walk per boundary size: the float64 data set is the same values widened, so both share a reference."""
    return hc.one_of_each_length(hc.boundary_lengths(dim), dim, seed=70 + dim, dtype=np.float32)


def boundary_case(dim, shape):
    """The data set that runs shape number `shape` -- the kernel is chosen by the data set's longest set, so it holds the
    boundary sizes up to the shape's limit -- and its pair list: all ordered pairs among the sizes up to 513, and each larger
    size against {1, R, 4096} in both orders (9 pairs touch the 4096-point set)."""
    Ls = hc.boundary_lengths(dim)
    R, G = hc.instantiations(dim)[shape]
    limit = hc.shape_limit(shape)
    nkeep = sum(L <= limit for L in Ls)   # (Ls ascends: the data set is its first nkeep sets)
    assert Ls[nkeep - 1] == limit
    nsmall = sum(L <= 513 for L in Ls[:nkeep])
    IJ = [tuple(p) for p in hc.all_ordered_pairs(nsmall)]
    partners = [Ls.index(L) for L in (1, R, hc.MAX_POINTS)]
    for k in range(nsmall, nkeep):
        IJ += [p for q in partners for p in ((k, q), (q, k))]
    IJ = np.array(sorted(set(IJ)), dtype=np.int64)
    assert np.any(IJ == Ls.index(hc.MAX_POINTS), axis=1).sum() <= 12
    return nkeep, IJ


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("dim", hc.DIMS)
def test_boundary_sizes(dim, shape, dtype):
    """The strip and group boundaries {1, R-1, R, R+1, 2R, GR-1, GR, GR+1, 2GR+1} of both shapes, 4095 and 4096, on the shape
    that the data set's longest member selects."""
    Ls, X = hc.boundary_lengths(dim), boundary_sets(dim)
    R, G = hc.instantiations(dim)[shape]
    assert {1, R - 1, R, R + 1, 2 * R, G * R - 1, G * R, G * R + 1, 2 * G * R + 1, 4095, 4096} <= set(Ls)
    nkeep, IJ = boundary_case(dim, shape)
    sub = X[:nkeep]
    assert max(map(len, sub)) == hc.shape_limit(shape) and (shape == 0) == (max(map(len, sub)) <= hc.SHORT)
    want = ref(("boundary", dim, shape), lambda: hc.hausdorff_pairs_host(sub, IJ))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs("hausdorff", [x.astype(dtype) for x in sub], IJ)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 3. outlier position
@pytest.mark.parametrize("dim, shape", [(2, 0), (2, 1), (1, 0), (3, 1), (4, 0)])
def test_outlier_position(dim, shape):
    """A base set of 2 G R + 1 points in a unit box and a partner that is the base plus noise of 1e-3.  Point p of the first set
    is moved far away (+100 on coordinate 0), for p at the strip and lane-group edges: the result is decided by that one row
    (one column in the other order), so a dropped row or column at an edge, or a missing direction, shows."""
    R, G = hc.instantiations(dim)[shape]
    L = 2 * G * R + 1
    assert (shape == 0) == (L <= hc.SHORT)
    rng = np.random.default_rng(80 + dim)
    base = rng.uniform(0.0, 1.0, (L, dim))
    partner = base + 1e-3 * rng.standard_normal((L, dim))
    ps = [0, R - 1, R, G * R - 1, G * R, 2 * G * R]
    X = [partner]
    for p in ps:
        x = base.copy()
        x[p, 0] += 100.0
        X.append(x)
    IJ = np.array([q for k in range(1, len(X)) for q in ((k, 0), (0, k))], dtype=np.int64)
    want = hc.hausdorff_pairs_host(X, IJ)
    assert np.all(want > 98.0) and len(np.unique(want)) == len(ps)
    assert hc.hausdorff_pair_host(base, partner) < 0.1
    got = pc.device_pairs("hausdorff", X, IJ)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------------------------- 4. set semantics
def test_set_semantics():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((300, 3))
    shuffled = x[rng.permutation(300)]
    dup = np.concatenate([x, x[rng.integers(0, 300, 45)]])
    sub = x[:170]
    X = [x, shuffled, dup, sub]
    IJ = np.array([[0, 1], [1, 0], [0, 2], [2, 0], [1, 2], [0, 3], [3, 0]], dtype=np.int64)
    got = pc.device_pairs("hausdorff", X, IJ)
    assert got[:5].tolist() == [0.0] * 5
    assert got[5] == got[6] > 0.0
    assert np.array_equal(got, hc.hausdorff_pairs_host(X, IJ))


# ----------------------------------------------------------------------------------------------- 5. PairSource forms
def fit_ref():
    """Every pair of the fit data set, [nx * nx]."""
    return ref("fit", lambda: pc.sym_matrix(hc.hausdorff_pairs_host, hc.fit_sets()).ravel())


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_ref()[IJ[:, 0] * len(hc.fit_sets()) + IJ[:, 1]])


def test_pair_source_forms():
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: ann.D), and positions into the pair list with the
    result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = hc.fit_sets()
    rng = np.random.default_rng(4)
    X[7] = X[3][rng.permutation(len(X[3]))]   # the same set, stored in another order
    nx = len(X)
    IJ = hc.all_ordered_pairs(nx)[::7]
    want = hc.hausdorff_pairs_host(X, IJ)
    eng = pc.bound("hausdorff", X)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, want)
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], hc.hausdorff_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, "hausdorff", **hc.FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], hc.hausdorff_pairs_host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], hc.hausdorff_pairs_host(X, ann.IJs[done]))


# ------------------------------------------------------------------------------------------------------ 6. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = hc.brute_sets()
    assert len(X) == 200 and all(x.shape[1] == 3 for x in X) and len({len(x) for x in X}) > 20
    bf = BruteForce(X, "hausdorff").fit()
    nx = len(X)
    T = pc.sym_matrix(hc.hausdorff_pairs_host, X)
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 7. fits
def test_fit_parity_with_the_cpu_pipeline(capsys):
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = hc.fit_sets()
    nx = len(X)
    ann = Annchor(X, "hausdorff", ols="lapack", **hc.FIT_CFG).fit()
    ora = O.OracleAnnchor(nx, fit_pairs, **hc.FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    # the default solver: whatever the graph lists is an exact distance, and no note about the triangle inequality
    dflt = Annchor(X, "hausdorff", **hc.FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(fit_pairs, nx)
    k = hc.FIT_CFG["n_neighbors"]
    print("is_metric=True, p_work=0.3: %d of %d neighbours differ from the exact graph; %d evaluations"
          % (compare_neighbor_graphs(exact[:2], dflt.neighbor_graph, k), nx * k, dflt.evals))


# ----------------------------------------------------------------------------------------------------------- 8. query
def test_query_with_other_sizes():
    """X is a 3-D array [240, 48, 2], Q a list of 20 sets of 30..70 points."""
    from annchor_amd import Annchor

    X = np.stack(hc.clustered_curves(240, 48, 48, 2, seed=33))
    Q = hc.clustered_curves(20, 30, 70, 2, seed=34)
    assert X.shape == (240, 48, 2) and min(map(len, Q)) >= 30 and max(map(len, Q)) <= 70 and len({len(q) for q in Q}) > 5
    both = list(X) + Q
    nx = len(X)
    pairs = lambda IJ: hc.hausdorff_pairs_host(both, IJ)
    ann = Annchor(X, "hausdorff", ols="lapack", **hc.FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, pairs, **hc.FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: pairs(np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5, p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# --------------------------------------------------------------------------------------------------- 9. loose objects
def test_loose_objects():
    from annchor_amd.distances import hausdorff

    rng = np.random.default_rng(6)
    xs = [rng.standard_normal((L, 3)) for L in (5, 40, 1, 130)]
    ys = [rng.standard_normal((L, 3)) for L in (17, 9, 33, 2)]
    assert hausdorff(xs[0], ys[0]) == hc.hausdorff_loop(xs[0], ys[0])
    assert hausdorff(ys[1], xs[1]) == hc.hausdorff_loop(ys[1], xs[1])
    assert np.array_equal(hausdorff.many(xs, ys), [hc.hausdorff_loop(x, y) for x, y in zip(xs, ys)])
    assert np.array_equal(hausdorff.one_to_many(xs[1], ys), [hc.hausdorff_loop(xs[1], y) for y in ys])
    # univariate members
    a, b = rng.standard_normal(12), rng.standard_normal(7)
    assert hausdorff(a, b) == hc.hausdorff_loop(a, b)


# --------------------------------------------------------------------------------------------------------- 10. limits
def test_limits():
    from annchor_amd import BruteForce, _native

    rng = np.random.default_rng(5)
    with pytest.raises(ValueError, match="hausdorff: set 0 has 4097 points"):
        BruteForce([rng.standard_normal((4097, 2)), rng.standard_normal((10, 2))], "hausdorff")
    with pytest.raises(ValueError, match="hausdorff: set 0 has dim 5"):
        BruteForce([rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], "hausdorff")
    with pytest.raises(ValueError, match="hausdorff: set 1 has dim 3, set 0 has dim 2"):
        BruteForce([rng.standard_normal((10, 2)), rng.standard_normal((10, 3))], "hausdorff")
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        v = rng.standard_normal((4097 + 10) * 2)
        with pytest.raises(_native.NativeError, match=r"error -4: .*4097.*1\.\.4096"):
            eng.set_point_sets(v, np.array([0, 4097]), np.array([4097, 10]), 2)
        with pytest.raises(_native.NativeError, match=r"error -4: .*dim 5"):
            eng.set_point_sets(v, np.array([0, 10]), np.array([10, 10]), 5)
        with pytest.raises(_native.NativeError, match=r"error -4: .*dim 0"):
            eng.set_point_sets(v, np.array([0, 10]), np.array([10, 10]), 0)
        with pytest.raises(_native.NativeError, match=r"error -1: .*empty"):
            eng.set_point_sets(v, np.array([0, 10]), np.array([10, 0]), 2)
        v[3] = np.nan
        with pytest.raises(_native.NativeError, match="error -1: .*non-finite"):
            eng.set_point_sets(v, np.array([0, 4096]), np.array([4096, 10]), 2)
        v[3] = np.inf
        with pytest.raises(_native.NativeError, match="error -1: .*non-finite"):
            eng.set_point_sets(v.astype(np.float32), np.array([0, 4096]), np.array([4096, 10]), 2)
        # 4096 points are taken
        v[3] = 0.0
        eng.set_point_sets(v, np.array([0, 4096]), np.array([4096, 10]), 2)
        x, y = v[:8192].reshape(4096, 2), v[8192:8212].reshape(10, 2)
        assert eng.metric_pairs(np.array([[0, 1], [1, 0]])).tolist() == [hc.hausdorff_pair_host(x, y)] * 2
    finally:
        eng.close()
