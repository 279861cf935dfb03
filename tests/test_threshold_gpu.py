"""EDR and LCSS on the device (csrc/seqdp.hip, EdrOp and LcssOp) against the host recurrences of threshold_cases.py.

Tolerance: none.  Every cell is a small integer that float64 holds exactly, and the final division is one correctly rounded
float64 operation on both sides; each comparison of distances below is np.array_equal.  Integer and saturating distances tie
heavily, so fits, brute-force graphs and queries are compared against the same pipeline fed bit-equal host distances, never
against an independently sorted graph."""
import numpy as np
import pytest

import pool_cases as pc
import seqdp_cases as sc
import test_seqdp_gpu as suite
import threshold_cases as tc
import wed_cases as wc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PARAMS = {"edr": [{"normalize": False}, {"normalize": True}], "lcss": [{"delta": None}, {"delta": 0}, {"delta": 5}]}
SPEC = {name: suite.spec(name, tc.HOSTS[name]) for name in PARAMS}
CASES = [pytest.param(name, kw, id="%s-%s" % (name, "-".join("%s%s" % kv for kv in kw.items()))) for name in PARAMS for kw in PARAMS[name]]


def boundary_data(name, dim):
    """One float32 grid series per boundary length (the float64 data set is the same values widened: one reference for both)."""
    return tc.grid_series(sc.boundary_lengths(name, dim), dim, seed=90 + dim, dtype=F32)


def count_ref(name, dim, shape, delta=None):
    """The corner cells of the boundary case: EDR's serve both values of `normalize`."""
    nkeep, IJ = sc.boundary_case(name, dim, shape)
    sub = boundary_data(name, dim)[:nkeep]
    measure = tc.Edr(tc.GRID_EPS[dim]) if name == "edr" else tc.Lcss(tc.GRID_EPS[dim], delta)
    return suite.ref((name, "boundary-count", dim, shape, delta), lambda: sc.pairs_host(sub, IJ, measure))


# ---------------------------------------------------------------------------------------------------- 1. small lengths
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name, kw", CASES)
def test_small_lengths(name, kw, dtype):
    """One grid series of dim 2 of each length 1..96, all 9216 ordered pairs: equal to the host, symmetric, zero on the diagonal."""
    X = tc.grid_series(range(1, 97), 2, seed=21, dtype=dtype)
    suite.small_lengths(SPEC[name], X, tuple(sorted(kw.items())) + (np.dtype(dtype).name,), eps=tc.GRID_EPS[2], **kw)


# ------------------------------------------------------------------------------------------------- 2. boundary lengths
@pytest.mark.parametrize("shape, dtype", [(0, F64), (0, F32), (1, F64), (2, F64), (2, F32)])
@pytest.mark.parametrize("dim", sc.DIMS)
@pytest.mark.parametrize("name, kw", CASES)
def test_boundary_lengths(name, kw, dim, shape, dtype):
    """The strip and group boundaries of every shape at this dim, 1, the limit and the limit minus 1 (seqdp_cases.boundary_case),
    on bounded data where differences of exactly eps occur and 20 % .. 80 % of the point pairs match; symmetric and zero on the
    diagonal on the same run."""
    eps = tc.GRID_EPS[dim]
    limit = sc.max_length(name, dim)
    R, G = sc.instantiations(name, dim)[shape]
    nkeep, IJ = sc.boundary_case(name, dim, shape)
    sub = boundary_data(name, dim)[:nkeep]
    assert max(map(len, sub)) == R * G and (shape < 2 or R * G == limit)
    assert 0.2 <= tc.match_share(sub, eps) <= 0.8
    count = count_ref(name, dim, shape, kw.get("delta"))
    want = tc.edr_finish(count, sub, IJ, kw["normalize"]) if name == "edr" else tc.lcss_finish(count, sub, IJ)
    assert np.all(np.isfinite(want))
    got = pc.device_pairs(name, [x.astype(dtype) for x in sub], IJ, eps=eps, **kw)
    assert np.array_equal(got, want)
    at = {(int(i), int(j)): k for k, (i, j) in enumerate(IJ)}
    assert all(got[k] == got[at[(j, i)]] for (i, j), k in at.items())
    assert all(got[k] == 0.0 for (i, j), k in at.items() if i == j)


# ------------------------------------------------------------------------------------ 3. against the device Levenshtein
def test_edr_at_eps_zero_is_the_device_levenshtein():
    X = tc.integer_sequences()
    strings = ["".join(wc.SYMBOLS[int(v)] for v in x) for x in X]
    IJ = pc.all_ordered_pairs(len(X))
    lev = pc.device_pairs("levenshtein", strings, IJ)
    assert lev.max() > 10
    assert np.array_equal(pc.device_pairs("edr", X, IJ, eps=0.0), lev)


# ----------------------------------------------------------------------------------------------------- 4. loose objects
def test_loose_objects():
    from annchor_amd import distances

    rng = np.random.default_rng(6)
    xs = [0.3 * np.cumsum(rng.standard_normal((L, 3)), axis=0) for L in (5, 40, 1, 130)]
    ys = [0.3 * np.cumsum(rng.standard_normal((L, 3)), axis=0) for L in (17, 9, 33, 2)]
    for f, loop, kw in ((distances.EDR(0.3), tc.edr_loop, {}), (distances.EDR(0.3, normalize=True), tc.edr_loop, {"normalize": True}),
                        (distances.LCSS(0.3), tc.lcss_loop, {}), (distances.LCSS(0.3, delta=4), tc.lcss_loop, {"delta": 4})):
        assert f(xs[0], ys[0]) == loop(xs[0], ys[0], 0.3, **kw)
        assert f(ys[1], xs[1]) == loop(ys[1], xs[1], 0.3, **kw)
        assert np.array_equal(f.many(xs, ys), [loop(x, y, 0.3, **kw) for x, y in zip(xs, ys)])
        assert np.array_equal(f.one_to_many(xs[1], ys), [loop(xs[1], y, 0.3, **kw) for y in ys])
        a, b = rng.standard_normal(12).round(1), rng.standard_normal(7).round(1)   # univariate members
        assert f(a, b) == loop(a, b, 0.3, **kw)
    f64 = np.float64
    assert distances.EDR(1.0)(f64([0, 0, 0]), f64([5])) == 3.0
    assert distances.EDR(0.5)(f64([1, 2, 3, 4]), f64([1.4, 3.5, 9])) == 2.0 == distances.EDR(0.5)(F32([1.4, 3.5, 9]), F32([1, 2, 3, 4]))
    assert distances.LCSS(0.0)(f64([1, 2, 3, 4]), f64([2, 4])) == 0.0 and distances.LCSS(0.0, delta=0)(f64([1, 2, 3, 4]), f64([2, 4])) == 1.0
    assert distances.LCSS(0.0, delta=1)(f64([1, 2, 3, 4]), f64([4, 1, 2])) == 1.0 - 2.0 / 3.0


# ------------------------------------------------------------------------------------------------------------ 5. limits
@pytest.mark.parametrize("name", ["edr", "lcss"])
def test_limits(name):
    """The host's refusals and the library's own behind them; a member of exactly the limit is taken."""
    from annchor_amd import _native

    rng = np.random.default_rng(5)
    L1, L3 = sc.max_length(name, 1), sc.max_length(name, 3)
    assert (L1, L3) == (2048, 1024)
    ok = {"func_kwargs": {"eps": 0.5}}
    for match, X, kw in [("%s: series 0 has %d points" % (name, L1 + 1), [rng.standard_normal(L1 + 1), rng.standard_normal(10)], ok),
                         ("%s: series 1 has %d points" % (name, L3 + 1), [rng.standard_normal((10, 3)), rng.standard_normal((L3 + 1, 3))], ok),
                         ("%s: series 0 has dim 5" % name, [rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], ok),
                         ("%s: series 1 has dim 3, series 0 has dim 2" % name, [rng.standard_normal((10, 2)), rng.standard_normal((10, 3))], ok),
                         ("%s: series 1 is empty" % name, [rng.standard_normal((10, 2)), np.zeros((0, 2))], ok),
                         ("%s: series 0 .*not finite" % name, [np.array([1.0, np.nan]), rng.standard_normal(10)], ok)] + \
                        [("%s: eps must be a finite real number >= 0" % name, [rng.standard_normal(10), rng.standard_normal(10)],
                          {"func_kwargs": {"eps": bad}}) for bad in (np.nan, np.inf, -0.5)]:
        suite.raises_value_error(match, X, name, **kw)
    v1, v3 = rng.standard_normal(L1 + 1 + 10), rng.standard_normal((L3 + 1 + 10) * 3)
    bad = v3.copy()
    bad[3] = np.nan
    eng = _native.Engine(0)
    setter = getattr(eng, "set_%s_series" % name)
    try:
        for match, args in [(r"error -4: .*%d.*1\.\.%d at dim 1" % (L1 + 1, L1), (v1, [0, L1 + 1], [L1 + 1, 10], 1, 0.5)),
                            (r"error -4: .*%d.*1\.\.%d at dim 3" % (L3 + 1, L3), (v3, [0, L3 + 1], [L3 + 1, 10], 3, 0.5)),
                            (r"error -4: .*dim 5", (v3, [0, 10], [10, 10], 5, 0.5)),
                            (r"error -1: .*empty", (v3, [0, 10], [10, 0], 3, 0.5)),
                            ("error -1: .*non-finite", (bad, [0, L3], [L3, 10], 3, 0.5))] + \
                           [(r"error -1: %s: the threshold eps" % name, (v3, [0, 10], [10, 10], 3, e)) for e in (np.nan, np.inf, -0.5)]:
            with pytest.raises(_native.NativeError, match=match):
                setter(args[0], np.array(args[1]), np.array(args[2]), args[3], args[4])
        # the limit itself is taken
        w = (rng.integers(0, 5, size=L1 + 10) * 0.5)
        setter(w, np.array([0, L1]), np.array([L1, 10]), 1, 0.5)
        assert eng.metric_pairs(np.array([[0, 1]]))[0] == tc.HOSTS[name]([w[:L1], w[L1:]], [[0, 1]], 0.5)[0]
    finally:
        eng.close()


# --------------------------------------------------------------------------------------- 6. fit, brute force and query
def fit_matrix(name, kw):
    """Every pair of the fit data and its 20 held-out members, [260 * 260]."""
    both = tc.fit_series() + tc.query_series()
    key = (name, "fit") + tuple(sorted(kw.items()))
    return suite.ref(key, lambda: pc.sym_matrix(lambda X, IJ: tc.HOSTS[name](X, IJ, **kw), both).ravel())


@pytest.mark.parametrize("name, kw", [pytest.param(n, tc.FIT_PARAMS[n][-1], id=n) for n in ("edr", "lcss")])
def test_fit_brute_force_and_query(name, kw, capsys):
    from annchor_amd import Annchor, BruteForce

    X, Q = tc.fit_series(), tc.query_series()
    nx, nall = len(X), len(X) + len(Q)
    T = fit_matrix(name, kw)

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

    # the is-metric note covers the two new classes
    Annchor(X, name, func_kwargs=kw, **pc.FIT_CFG)
    assert "triangle inequality" in capsys.readouterr().err
    dev = Annchor(X, name, func_kwargs=kw, is_metric=False, ols="lapack", **pc.FIT_CFG)
    assert "triangle inequality" not in capsys.readouterr().err
    dev.fit()
    host = Annchor(X, name, func_kwargs=kw, is_metric=False, ols="lapack", get_exact_ijs=evaluator, **pc.FIT_CFG).fit()
    assert dev.evals == host.evals
    assert np.array_equal(dev.neighbor_graph[1], host.neighbor_graph[1])
    assert np.array_equal(dev.neighbor_graph[0], host.neighbor_graph[0])
    idx, dist = dev.neighbor_graph
    NN = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), pairs(NN))
    # brute force: the host's exact graph
    bf = BruteForce(X, name, func_kwargs=kw).fit()
    oi, od, _ = O.brute_force(pairs, nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)
    # 20 held-out members
    gi, gd = dev.query(Q, nn=5, p_work=0.3)
    hi, hd = host.query(Q, nn=5, p_work=0.3, get_exact_query_ijs=query_evaluator)
    assert dev.query_evals == host.query_evals
    assert np.array_equal(gd, hd)
    assert np.array_equal(gi, hi)
    QI = np.stack([np.repeat(np.arange(len(Q)) + nx, gi.shape[1]), np.asarray(gi).ravel()], axis=1)
    assert np.array_equal(np.asarray(gd).ravel(), pairs(QI))
