"""DTW and Frechet on members of 5 .. 64 coordinates per point on the device (csrc/seqwide.hip, k_seqwide) against the host sweep of
seqdp_cases.py, whose _sq loops over any dim.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import pool_cases as pc
import radius_cases as rc
import seqdp_cases as sc
import threshold_cases as tc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ref = pc.ref_cache()
MEASURES = [("dtw", {"window": None}), ("dtw", {"window": 0}), ("dtw", {"window": 5}), ("dtw", {"window": 64}), ("frechet", {})]


def host(name, X, IJ, kw):
    return sc.dtw_pairs_host(X, IJ, **kw) if name == "dtw" else sc.frechet_pairs_host(X, IJ)


def check(key, name, kw, X, dtype):
    """All ordered pairs of X (float32-representable values) on the device in `dtype` against the host; the key leaves dtype
    out on purpose: both dtypes hold the same values and share one reference."""
    IJ = pc.all_ordered_pairs(len(X))
    want = ref(key, lambda: host(name, X, IJ, kw))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs(name, [x.astype(dtype) for x in X], IJ, wide=True, **kw)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("name, kw", MEASURES)
@pytest.mark.parametrize("dim", [5, 8, 13, 64])
def test_tile_edges(dim, name, kw, dtype):
    """k_seqwide cuts the rows into strips of 64 and a strip's anti-diagonal steps into phases of 48 (not the issue's column
    tiles of 32): the lengths are 1, 2, {47, 48, 49}, {63, 64, 65}, {127, 128, 129} and 200 (four strips, nine phases).  dim 13 is
    no multiple of the 16-coordinate chunk, dim 64 is four chunks.  window = 0 and 5 skip phases, 64 skips some."""
    X = sc.one_of_each_length([1, 2, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200], dim, seed=70 + dim, dtype=F32)
    check(("edges", dim, name, kw.get("window")), name, kw, X, dtype)


@pytest.mark.parametrize("name, kw", [("dtw", {"window": None}), ("dtw", {"window": 7}), ("frechet", {})])
@pytest.mark.parametrize("dim, dtype", [(64, F32), (5, F64)])
def test_ceiling(dim, dtype, name, kw):
    """Members of 1024, 1023 and 1 points, the nine ordered pairs."""
    X = sc.one_of_each_length([1024, 1023, 1], dim, seed=80 + dim, dtype=F32)
    check(("ceiling", dim, name, kw.get("window")), name, kw, X, dtype)


def large_magnitudes():
    rng = np.random.default_rng(90)
    return [1e6 + rng.standard_normal((L, 13)) for L in (70, 50, 9)]


def test_large_magnitudes():
    """Coordinates near 1e6 plus unit noise at dim 13: a difference has about 33 significant bits, so its square and the sums are
    all rounded.  On this input the pairwise order of np.sum changes the bits of 24 % of the c(i, j), and a sum with fused
    multiply-adds (emulated in exact rational arithmetic) those of 37 of 100 sampled cells: checked on the CPU when the test was
    written, and the np.sum variant again here.  A path crosses some 70 cells, so either variant changes the distance."""
    X = large_magnitudes()
    a, b = X[0][:, None, :], X[1][None, :, :]
    assert np.mean(np.sum((a - b) * (a - b), axis=-1) != sc._sq(a, b)) > 0.1
    for name, kw in (("dtw", {"window": None}), ("dtw", {"window": 3}), ("frechet", {})):
        IJ = pc.all_ordered_pairs(len(X))
        assert np.array_equal(pc.device_pairs(name, X, IJ, wide=True, **kw), host(name, X, IJ, kw))


def test_opt_in():
    from annchor_amd import BruteForce, _native, distances

    rng = np.random.default_rng(91)
    X3 = sc.one_of_each_length([1, 40, 130, 600], 3, seed=92)
    IJ = pc.all_ordered_pairs(len(X3))
    for name, kw in (("dtw", {"window": 4}), ("frechet", {})):
        assert np.array_equal(pc.device_pairs(name, X3, IJ, wide=True, **kw), pc.device_pairs(name, X3, IJ, **kw))
    X5 = [rng.standard_normal((10, 5)), rng.standard_normal((12, 5))]
    for metric, match in [(distances.DTW(), "dtw: series 0 has dim 5; dim 1 .. 4"), ("dtw", "dtw: series 0 has dim 5; dim 1 .. 4"),
                          (distances.Frechet(), "frechet: curve 0 has dim 5; dim 1 .. 4"), ("frechet", "frechet: curve 0 has dim 5; dim 1 .. 4")]:
        with pytest.raises(ValueError, match=match):
            BruteForce(X5, metric)
    x, y = X5
    assert distances.DTW(wide=True)(x, y) == tc.dtw_loop(x, y) == distances.DTW(wide=True)(y, x)
    v = rng.standard_normal((1025 + 10) * 5)
    bad = v.copy()
    bad[3] = np.nan
    eng = _native.Engine(0)
    try:
        for setter in (eng.set_series_wide, eng.set_curves_wide):
            for match, args in [(r"error -4: .*dim 4.*5\.\.64", (v, [0, 10], [10, 10], 4)),
                                (r"error -4: .*dim 65.*5\.\.64", (np.zeros(20 * 65), [0, 10], [10, 10], 65)),
                                (r"error -4: .*1025.*1\.\.1024 at dim 5", (v, [0, 1025], [1025, 10], 5)),
                                (r"error -1: .*empty", (v, [0, 10], [10, 0], 5)),
                                ("error -1: .*non-finite", (bad, [0, 1024], [1024, 10], 5))]:
                with pytest.raises(_native.NativeError, match=match):
                    setter(args[0], np.array(args[1]), np.array(args[2]), args[3])
    finally:
        eng.close()


def fit_data():
    return sc.clustered_curves(160, 20, 60, 13, seed=93), sc.clustered_curves(20, 20, 60, 13, seed=94)


def test_dtw_fit_brute_force_and_query():
    """test_dtw_nd_gpu.py::test_fit_brute_force_and_query at dim 13: the device fit against the same fit over the host matrix."""
    from annchor_amd import Annchor, BruteForce

    X, Q = fit_data()
    nx, nall = len(X), len(X) + len(Q)
    T = ref(("fit", "dtw"), lambda: pc.sym_matrix(sc.dtw_pairs_host, X + Q).ravel())
    kw = {"wide": True}

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(T[IJ[:, 0] * nall + IJ[:, 1]])

    def query_evaluator(f, Xs, Z, IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        rows = IJ[:, 0] if len(Xs) == nx else np.asarray(host_fit.A, dtype=np.int64)[IJ[:, 0]]
        return pairs(np.stack([rows, IJ[:, 1] + nx], axis=1))

    dev = Annchor(X, "dtw", func_kwargs=kw, is_metric=False, ols="lapack", **pc.FIT_CFG).fit()
    host_fit = Annchor(X, "dtw", func_kwargs=kw, is_metric=False, ols="lapack", get_exact_ijs=lambda f, Xs, IJ: pairs(IJ), **pc.FIT_CFG).fit()
    assert dev.evals == host_fit.evals
    assert np.array_equal(dev.neighbor_graph[1], host_fit.neighbor_graph[1])
    assert np.array_equal(dev.neighbor_graph[0], host_fit.neighbor_graph[0])
    bf = BruteForce(X, "dtw", func_kwargs=kw).fit()
    oi, od, _ = O.brute_force(pairs, nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)
    gi, gd = dev.query(Q, nn=5, p_work=0.3)
    hi, hd = host_fit.query(Q, nn=5, p_work=0.3, get_exact_query_ijs=query_evaluator)
    assert dev.query_evals == host_fit.query_evals
    assert np.array_equal(gd, hd)
    assert np.array_equal(gi, hi)


def test_frechet_radius_graph():
    """Frechet(wide=True) is a metric: the anchor rounds and the radius forms, against brute force and the host matrix."""
    from annchor_amd import Annchor, BruteForce, distances

    X = fit_data()[0]
    M = ref(("fit", "frechet"), lambda: pc.sym_matrix(sc.frechet_pairs_host, X))
    r = float(np.percentile(M[np.triu_indices(len(X), 1)], 5))
    g = Annchor(X, "frechet", func_kwargs={"wide": True}, **pc.FIT_CFG).radius_graph(r)
    gb = BruteForce(X, distances.Frechet(wide=True)).radius_graph(r)
    want = rc.graph_from_matrix(M, r)
    assert rc.same_graph((g.indptr, g.indices, g.distances), want)
    assert rc.same_graph((gb.indptr, gb.indices, gb.distances), want)
