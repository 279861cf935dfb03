"""ERP and TWE on members of 5 .. 64 coordinates per point on the device (csrc/editwide.hip, k_editwide) against the host sweep of
seqdp_cases.py, whose _dist loops over any dim.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import elastic_cases as ec
import erp_cases as erc
import pool_cases as pc
import radius_cases as rc
import seqdp_cases as sc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ref = pc.ref_cache()
MEASURES = [("erp", {}), ("erp", {"gap": 0.37}), ("twe", {"nu": 0.37, "lam": 0.21}), ("twe", {"nu": 0.0, "lam": 0.5})]
HOST = {"erp": sc.erp_pairs_host, "twe": sc.twe_pairs_host}


def check(key, name, kw, X, dtype):
    """All ordered pairs of X (float32-representable values) on the device in `dtype` against the host; the key leaves dtype out
    on purpose: both dtypes hold the same values and share one reference.  Returns the matrix."""
    IJ = pc.all_ordered_pairs(len(X))
    want = ref((key, name, tuple(kw.values())), lambda: HOST[name](X, IJ, **kw))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs(name, [x.astype(dtype) for x in X], IJ, wide=True, **kw)
    assert np.array_equal(got, want)
    return got.reshape(len(X), len(X))


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("name, kw", MEASURES)
@pytest.mark.parametrize("dim", [5, 13, 64])
def test_tile_edges(dim, name, kw, dtype):
    """k_editwide keeps k_seqwide's strips of 64 rows and phases of 48 steps, so the lengths are the issue's.  The chunk is 16
    coordinates in float32 and 8 in float64: dims 5 and 13 are multiples of neither, dim 64 is four and eight chunks."""
    X = sc.one_of_each_length([1, 2, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200], dim, seed=70 + dim, dtype=F32)
    M = check(("edges", dim), name, kw, X, dtype)
    assert np.all(np.diag(M) == 0.0) and np.array_equal(M, M.T)


@pytest.mark.parametrize("name, kw", [MEASURES[1], MEASURES[2]])
@pytest.mark.parametrize("dim, dtype", [(64, F32), (5, F64)])
def test_ceiling(dim, dtype, name, kw):
    """Members of 1024, 1023 and 1 points, the nine ordered pairs."""
    check(("ceiling", dim), name, kw, sc.one_of_each_length([1024, 1023, 1], dim, seed=80 + dim, dtype=F32), dtype)


@pytest.mark.parametrize("name, kw", [("erp", {"gap": 0.0}), MEASURES[2]])
def test_rounding_order(name, kw):
    """Coordinates near 1e6 plus unit noise at dim 13.  Between two one-point members both measures are dist(x[0], y[0]) itself,
    and np.sum's pairwise order changes its bits on 8.0 % of the 552 such pairs (computed on the CPU for this generator;
    asserted > 5 % here), so a reordered or fused sum cannot pass; the longer members take that arithmetic through the sweep."""
    rng = np.random.default_rng(95)
    X = [1e6 + rng.standard_normal((1, 13)) for _ in range(24)] + [1e6 + rng.standard_normal((L, 13)) for L in (70, 50, 9)]
    P = np.concatenate(X[:24])
    d = P[:, None, :] - P[None, :, :]
    off = ~np.eye(24, dtype=bool)
    assert np.mean((np.sqrt(np.sum(d * d, axis=-1)) != sc._dist(P[:, None, :], P[None, :, :]))[off]) > 0.05
    M = check("rounding", name, kw, X, F64)
    assert np.array_equal(M[:24, :24][off], sc._dist(P[:, None, :], P[None, :, :])[off])


def test_opt_in_and_limits():
    from annchor_amd import BruteForce, _native, distances

    X3 = sc.one_of_each_length([1, 40, 130, 600], 3, seed=92)
    IJ = pc.all_ordered_pairs(len(X3))
    for name, kw in MEASURES:
        assert np.array_equal(pc.device_pairs(name, X3, IJ, wide=True, **kw), pc.device_pairs(name, X3, IJ, **kw))
    rng = np.random.default_rng(91)
    x, y = X5 = [rng.standard_normal((10, 5)), rng.standard_normal((12, 5))]
    for metric in (distances.ERP(), "erp", distances.TWE(), "twe"):
        with pytest.raises(ValueError, match="%s: series 0 has dim 5; dim 1 .. 4" % getattr(metric, "name", metric)):
            BruteForce(X5, metric)
    erp, twe = distances.ERP(0.37, wide=True), distances.TWE(0.37, 0.21, wide=True)
    assert erp(x, y) == erc.erp_loop(x, y, 0.37) == erp(y, x) == erp.many([x], [y])[0] == erp.one_to_many(y, [x])[0]
    assert twe(x, y) == ec.twe_loop(x, y, 0.37, 0.21) == twe(y, x) == twe.many([x], [y])[0] == twe.one_to_many(y, [x])[0]
    v = rng.standard_normal((1025 + 10) * 5)
    bad = v.copy()
    bad[3] = np.nan
    eng = _native.Engine(0)
    try:
        ok = (v, [0, 10], [10, 10], 5)
        for setter, good, refused in ((eng.set_erp_series_wide, (0.0,), [("erp: the gap value", (np.nan,)), ("erp: the gap value", (np.inf,))]),
                                      (eng.set_twe_series_wide, (0.001, 1.0),
                                       [("twe: the stiffness nu", (-1.0, 1.0)), ("twe: the stiffness nu", (np.nan, 1.0)),
                                        ("twe: the penalty lam", (0.001, -1.0)), ("twe: the penalty lam", (0.001, np.inf))])):
            for match, args, extra in [(r"error -4: .*dim 4.*5\.\.64", (v, [0, 10], [10, 10], 4), good),
                                       (r"error -4: .*dim 65.*5\.\.64", (np.zeros(20 * 65), [0, 10], [10, 10], 65), good),
                                       (r"error -4: .*1025.*1\.\.1024 at dim 5", (v, [0, 1025], [1025, 10], 5), good),
                                       (r"error -1: .*empty", (v, [0, 10], [10, 0], 5), good),
                                       ("error -1: .*non-finite", (bad, [0, 1024], [1024, 10], 5), good)] \
                    + [("error -1: " + words, ok, extra) for words, extra in refused]:
                with pytest.raises(_native.NativeError, match=match):
                    setter(args[0], np.array(args[1]), np.array(args[2]), args[3], *extra)
    finally:
        eng.close()


def fit_data():
    return sc.clustered_curves(160, 20, 60, 13, seed=93), sc.clustered_curves(20, 20, 60, 13, seed=94)


def test_erp_fit_brute_force_and_query():
    """test_seqwide_gpu.py::test_dtw_fit_brute_force_and_query under ERP, a metric: is_metric stays at its default."""
    from annchor_amd import Annchor, BruteForce

    X, Q = fit_data()
    nx, nall = len(X), len(X) + len(Q)
    T = ref(("fit", "erp"), lambda: pc.sym_matrix(sc.erp_pairs_host, X + Q).ravel())
    kw = {"wide": True}

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(T[IJ[:, 0] * nall + IJ[:, 1]])

    def query_evaluator(f, Xs, Z, IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        rows = IJ[:, 0] if len(Xs) == nx else np.asarray(host_fit.A, dtype=np.int64)[IJ[:, 0]]
        return pairs(np.stack([rows, IJ[:, 1] + nx], axis=1))

    dev = Annchor(X, "erp", func_kwargs=kw, ols="lapack", **pc.FIT_CFG).fit()
    host_fit = Annchor(X, "erp", func_kwargs=kw, ols="lapack", get_exact_ijs=lambda f, Xs, IJ: pairs(IJ), **pc.FIT_CFG).fit()
    assert dev.evals == host_fit.evals
    assert np.array_equal(dev.neighbor_graph[1], host_fit.neighbor_graph[1]) and np.array_equal(dev.neighbor_graph[0], host_fit.neighbor_graph[0])
    bf = BruteForce(X, "erp", func_kwargs=kw).fit()
    oi, od, _ = O.brute_force(pairs, nx)
    assert np.array_equal(bf.neighbor_graph[1], od) and np.array_equal(bf.neighbor_graph[0], oi)
    gi, gd = dev.query(Q, nn=5, p_work=0.3)
    hi, hd = host_fit.query(Q, nn=5, p_work=0.3, get_exact_query_ijs=query_evaluator)
    assert dev.query_evals == host_fit.query_evals
    assert np.array_equal(gd, hd) and np.array_equal(gi, hi)


def test_twe_radius_graph():
    """TWE(wide=True) is a metric: the anchor rounds and the radius forms, against brute force and the host matrix."""
    from annchor_amd import Annchor, BruteForce, distances

    X = fit_data()[0]
    M = ref(("fit", "twe"), lambda: pc.sym_matrix(sc.twe_pairs_host, X))
    r = float(np.percentile(M[np.triu_indices(len(X), 1)], 5))
    g = Annchor(X, "twe", func_kwargs={"wide": True}, **pc.FIT_CFG).radius_graph(r)
    gb = BruteForce(X, distances.TWE(wide=True)).radius_graph(r)
    want = rc.graph_from_matrix(M, r)
    assert rc.same_graph((g.indptr, g.indices, g.distances), want)
    assert rc.same_graph((gb.indptr, gb.indices, gb.distances), want)


@pytest.mark.parametrize("steps", [[("erp", 5, {"wide": True}), ("erp", 2, {})],
                                   [("twe", 6, {"wide": True}), ("dtw", 5, {"wide": True}), ("erp", 5, {"wide": True})]])
def test_rebinding(steps):
    """One engine bound in turn: every later binding gives a fresh engine's values, so neither the per-point costs nor curve_dim
    leak from one binding to the next."""
    from annchor_amd.utils import get_function_from_input

    eng = pc.bound(steps[0][0], sc.one_of_each_length([70, 3, 130], steps[0][1], seed=96), **steps[0][2])
    try:
        for k, (name, dim, kw) in enumerate(steps[1:]):
            X = sc.one_of_each_length([5, 90, 66, 1], dim, seed=97 + k)
            IJ = pc.all_ordered_pairs(len(X))
            get_function_from_input(name, kw).bind(eng, X)
            assert np.array_equal(eng.metric_pairs(IJ), pc.device_pairs(name, X, IJ, **kw))
    finally:
        eng.close()
