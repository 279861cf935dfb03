"""The earth mover's distance between point clouds on the device (k_emd_points, csrc/emd.hip) against the oracle's exact solver
(emd_points_cases.emd_pairs_host).

Tolerance: atol = 1e-11 with rtol = 0, the project's bar for wide solves (test_wasserstein_wide_gpu.py), on data of that test's
scale: coordinates in [0, 10).  Both sides are LP optima in floating point, so values are compared with the tolerance; what the
definition promises exactly -- symmetry, zeros, purity, one value per pair whatever the pair source -- is compared bit for bit.
A solve that runs into its pivot cap or meets a broken tree writes NaN (the `fail` flag is not readable from the host, the NaN
is), so a NaN anywhere is a failure.  Every comparison prints the largest difference it saw."""
import numpy as np
import pytest

import emd_points_cases as ec
import pool_cases as pc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()


def close(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert not np.any(np.isnan(got)), "%s: NaN (a failed solve)" % label
    worst = float(np.max(np.abs(got - want))) if got.size else 0.0
    print("%s: largest difference from the oracle %.3g over %d values" % (label, worst, got.size))
    assert worst <= ec.ATOL, "%s: %.3g" % (label, worst)


def device_table(X):
    """Every ordered pair on the device, each in its own order, [nx, nx]."""
    nx = len(X)
    return pc.device_pairs("emd", X, pc.all_ordered_pairs(nx)).reshape(nx, nx)


def host_table(X):
    return ec.sym_table(lambda IJ: ec.emd_pairs_host(X, IJ), len(X))


# ------------------------------------------------------------------------------------------------- 1. slot boundaries
SLOT_SIZES = [(1, 1), (1, 2), (1, 63), (1, 64), (1, 128), (32, 32), (32, 33), (64, 64), (64, 65), (96, 96), (96, 97), (127, 128),
              (128, 128)]


def test_slot_boundaries():
    """Node counts on both sides of every slot boundary (64, 128, 192) and the largest solve, each pair in both orders."""
    X = ec.random_clouds([L for nm in SLOT_SIZES for L in nm], 2, seed=11)
    IJ = np.array([q for k in range(len(SLOT_SIZES)) for q in ((2 * k, 2 * k + 1), (2 * k + 1, 2 * k))], dtype=np.int64)
    assert [(len(X[i]), len(X[j])) for i, j in IJ[::2]] == SLOT_SIZES
    got = pc.device_pairs("emd", X, IJ)
    close(got, ec.emd_pairs_host(X, IJ), "slot boundaries")
    assert np.array_equal(got[::2], got[1::2])
    assert np.all(got > 0.0)


# ------------------------------------------------------------------------------------------------------ 2. small sizes
@pytest.mark.parametrize("dim", ec.DIMS)
def test_small_sizes(dim):
    """40 clouds of 1 .. 48 points, all ordered pairs, bound as float32 and as the same values widened to float64."""
    rng = np.random.default_rng(20 + dim)
    sizes = np.concatenate([[1, 1, 2, 48, 48], rng.integers(1, 49, 35)])
    X32 = ec.random_clouds(sizes, dim, seed=30 + dim, dtype=np.float32)
    X64 = [x.astype(np.float64) for x in X32]
    assert len(X32) == 40
    want = ref(("small", dim), lambda: host_table(X64))
    T32, T64 = device_table(X32), device_table(X64)
    close(T64, want, "small sizes, dim %d, float64" % dim)
    close(T32, want, "small sizes, dim %d, float32" % dim)
    assert np.array_equal(T64, T64.T) and np.array_equal(T32, T32.T)
    assert np.array_equal(T32, T64)
    assert np.all(np.diag(T64) == 0.0)


# ----------------------------------------------------------------------------------------------- 3. degenerate geometry
def degenerate_clouds(kind):
    rng = np.random.default_rng(40)
    if kind == "lattice2":
        return ec.lattice_clouds((128, 128, 100, 64, 37, 5, 128, 65), 2, seed=41)
    if kind == "lattice3":
        return ec.lattice_clouds((128, 127, 96, 64, 33, 2, 128), 3, seed=42)
    if kind == "collinear":
        # points on one line through the box, at multiples of 1/8 along it: ties and triangle equalities everywhere
        a, d = np.array([1.0, 2.0, 0.5]), np.array([0.5, 0.25, 0.75])
        return [a + (rng.integers(0, 80, L) / 8.0)[:, None] * d for L in (50, 70, 128, 128, 9)]
    if kind == "copies":
        return [np.tile([1.5, 2.5], (50, 1)), np.tile([7.0, 0.25], (70, 1)), np.tile([1.5, 2.5], (70, 1))]
    assert kind == "star"
    return [rng.random((1, 2)) * 10, rng.random((128, 2)) * 10, rng.random((1, 2)) * 10]


@pytest.mark.parametrize("kind", ["lattice2", "lattice3", "collinear", "copies", "star"])
def test_degenerate_geometry(kind):
    X = degenerate_clouds(kind)
    T = device_table(X)
    close(T, host_table(X), kind)
    assert np.array_equal(T, T.T)
    if kind == "copies":
        assert abs(T[0, 1] - np.sqrt(5.5 * 5.5 + 2.25 * 2.25)) <= ec.ATOL and T[0, 2] == 0.0


# --------------------------------------------------------------------------------------------------------- 4. zeros
@pytest.mark.parametrize("dim", ec.DIMS)
def test_zeros(dim):
    """The pairs (i, i), a permuted copy, a permuted copy of a cloud with duplicates: exactly 0.0, in both orders."""
    rng = np.random.default_rng(50 + dim)
    X = ec.random_clouds((1, 2, 37, 64, 100, 128), dim, seed=51 + dim)
    nbase = len(X)
    IJ = [(i, i) for i in range(nbase)]
    for i in range(nbase):
        X.append(X[i][rng.permutation(len(X[i]))])
        IJ += [(i, len(X) - 1), (len(X) - 1, i)]
    for L in (40, 128):
        base = rng.random((L // 4, dim)) * 10
        dup = base[rng.integers(0, len(base), L)]           # every point several times
        X += [dup, dup[rng.permutation(L)]]
        IJ += [(len(X) - 2, len(X) - 1), (len(X) - 1, len(X) - 2), (len(X) - 1, len(X) - 1)]
    lat = ec.lattice_clouds((128,), min(dim, 3), seed=52)[0]
    lat = np.concatenate([lat, np.zeros((128, dim - lat.shape[1]))], axis=1)
    X += [lat, lat[rng.permutation(128)]]
    IJ += [(len(X) - 2, len(X) - 1), (len(X) - 1, len(X) - 2)]
    got = pc.device_pairs("emd", X, np.array(IJ, dtype=np.int64))
    assert got.tolist() == [0.0] * len(IJ)
    assert not np.any(np.signbit(got))


# ------------------------------------------------------------------------------------------------ 5. PairSource forms
def fit_clouds():
    """160 clouds of dim 2 in six shape clusters, 20 .. 60 points; member 7 is member 3 stored in another order."""
    X = ec.shape_clouds(160, 20, 60, 2, seed=61)
    X[7] = X[3][np.random.default_rng(4).permutation(len(X[3]))]
    return X


def fit_table():
    """The device's value of every ordered pair of fit_clouds(), computed once with metric_pairs."""
    return ref("fit table", lambda: device_table(fit_clouds()))


def fit_pairs(IJ):
    IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
    return np.asarray(fit_table()[IJ[:, 0], IJ[:, 1]])


def test_pair_source_forms():
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows: pick_anchors_selected and ann.D), and positions into the pair
    list with the result written to RefineApprox / not_computed_mask: one value per pair, the table's."""
    from annchor_amd import Annchor, _native

    X = fit_clouds()
    nx = len(X)
    T = fit_table()
    assert np.array_equal(T, T.T) and T[3, 7] == 0.0 and np.all(np.diag(T) == 0.0)
    rng = np.random.default_rng(62)
    S = rng.integers(0, nx, (600, 2))
    close(T[S[:, 0], S[:, 1]], ec.emd_pairs_host(X, S), "fit table, 600 sampled pairs")
    eng = pc.bound("emd", X)
    IJ = pc.all_ordered_pairs(nx)[::7][::-1]
    assert np.array_equal(eng.metric_pairs(IJ), fit_pairs(IJ))
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    assert np.array_equal(D[:, 0], T[3]) and np.array_equal(D[:, 1], T[100])
    ann = Annchor(X, "emd", **pc.FIT_CFG).fit()
    for col, a in enumerate(np.asarray(ann.A)):
        assert np.array_equal(ann.D[:, col], T[a])
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], fit_pairs(ann.IJs[done]))


# ---------------------------------------------------------------------------------------------------------- 6. purity
def test_purity():
    """A pair's value depends on the pair alone: loose clouds, and the same clouds inside a data set whose bounding box is 100
    times wider, give the same bits."""
    from annchor_amd.distances import emd

    rng = np.random.default_rng(70)
    xs = ec.random_clouds((5, 40, 1, 128, 33, 64), 3, seed=71)
    ys = ec.random_clouds((17, 40, 33, 2, 33, 65), 3, seed=72)
    loose = emd.many(xs, ys)
    close(loose, [ec.emd_pair_host(x, y) for x, y in zip(xs, ys)], "loose clouds")
    assert emd(xs[1], ys[1]) == loose[1] and emd(ys[1], xs[1]) == loose[1]
    assert np.array_equal(emd.one_to_many(xs[3], ys), pc.device_pairs("emd", [xs[3]] + ys, [(0, k + 1) for k in range(len(ys))]))
    wide = [rng.random((int(L), 3)) * 1000 for L in rng.integers(1, 129, 30)]
    big = wide[:15] + xs + wide[15:] + ys
    lo, hi = np.concatenate(xs + ys).min(0), np.concatenate(xs + ys).max(0)
    blo, bhi = np.concatenate(big).min(0), np.concatenate(big).max(0)
    assert np.all(bhi - blo > 99 * (hi - lo))
    IJ = np.array([(15 + t, 15 + len(xs) + 15 + t) for t in range(len(xs))], dtype=np.int64)
    inside = pc.device_pairs("emd", big, np.concatenate([IJ, IJ[:, ::-1]]))
    assert np.array_equal(inside[:len(xs)], loose) and np.array_equal(inside[len(xs):], loose)
    # univariate members
    a, b = rng.random(12) * 10, rng.random(7) * 10
    assert abs(emd(a, b) - ec.emd_1d_closed_form(a, b)) <= ec.ATOL


# ------------------------------------------------------------------------------------------------------ 7. BruteForce
def test_brute_force():
    from annchor_amd import BruteForce

    X = ec.shape_clouds(160, 16, 48, 3, seed=81)
    nx = len(X)
    assert nx == 160 and all(x.shape[1] == 3 for x in X) and len({len(x) for x in X}) > 20
    bf = BruteForce(X, "emd").fit()
    T = device_table(X)
    close(T, host_table(X), "brute-force table")
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 8. fits
def test_fit_parity_with_the_cpu_pipeline(capsys):
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = fit_clouds()
    nx = len(X)
    fit_table()
    ann = Annchor(X, "emd", ols="lapack", **pc.FIT_CFG).fit()
    ora = O.OracleAnnchor(nx, fit_pairs, **pc.FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    # the default solver: whatever the graph lists is the table's value, and no note about the triangle inequality
    capsys.readouterr()
    dflt = Annchor(X, "emd", **pc.FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(fit_pairs, nx)
    k = pc.FIT_CFG["n_neighbors"]
    print("is_metric=True, p_work=0.3: %d of %d neighbours differ from the exact graph; %d evaluations"
          % (compare_neighbor_graphs(exact[:2], dflt.neighbor_graph, k), nx * k, dflt.evals))


# ----------------------------------------------------------------------------------------------------------- 9. query
def test_query_with_other_sizes():
    """X is a 3-D array [160, 32, 2], Q a list of 20 clouds of 10 .. 60 points."""
    from annchor_amd import Annchor

    X = np.stack(ec.shape_clouds(160, 32, 32, 2, seed=91))
    Q = ec.shape_clouds(20, 10, 60, 2, seed=92)
    assert X.shape == (160, 32, 2) and min(map(len, Q)) >= 10 and max(map(len, Q)) <= 60 and len({len(q) for q in Q}) > 5
    nx = len(X)
    T = device_table(list(X) + Q)
    pairs = lambda IJ: T[IJ[:, 0], IJ[:, 1]]
    ann = Annchor(X, "emd", ols="lapack", **pc.FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, pairs, **pc.FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: pairs(np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5, p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# --------------------------------------------------------------------------------------------------------- 10. limits
def test_limits():
    from annchor_amd import BruteForce, _native

    rng = np.random.default_rng(5)
    with pytest.raises(ValueError, match="emd: cloud 0 has 129 points"):
        BruteForce([rng.random((129, 2)), rng.random((10, 2))], "emd")
    with pytest.raises(ValueError, match="emd: cloud 0 has dim 5"):
        BruteForce([rng.random((10, 5)), rng.random((10, 5))], "emd")
    with pytest.raises(ValueError, match="emd: cloud 1 has dim 3, cloud 0 has dim 2"):
        BruteForce([rng.random((10, 2)), rng.random((10, 3))], "emd")
    with pytest.raises(ValueError, match="emd: cloud 1 is empty"):
        BruteForce([rng.random((10, 2)), np.zeros((0, 2))], "emd")
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        v = rng.random((129 + 10) * 2) * 10
        with pytest.raises(_native.NativeError, match=r"error -4: .*129.*1\.\.128"):
            eng.set_clouds(v, np.array([0, 129]), np.array([129, 10]), 2)
        with pytest.raises(_native.NativeError, match=r"error -4: .*dim 5"):
            eng.set_clouds(v, np.array([0, 10]), np.array([10, 10]), 5)
        with pytest.raises(_native.NativeError, match=r"error -1: .*empty"):
            eng.set_clouds(v, np.array([0, 10]), np.array([10, 0]), 2)
        v[3] = np.nan
        with pytest.raises(_native.NativeError, match="error -1: .*non-finite"):
            eng.set_clouds(v, np.array([0, 128]), np.array([128, 10]), 2)
        # 128 points are taken
        v[3] = 0.0
        eng.set_clouds(v, np.array([0, 128]), np.array([128, 10]), 2)
        x, y = v[:256].reshape(128, 2), v[256:276].reshape(10, 2)
        got = eng.metric_pairs(np.array([[0, 1], [1, 0]]))
        assert got[0] == got[1] and abs(got[0] - ec.emd_pair_host(x, y)) <= ec.ATOL
    finally:
        eng.close()
