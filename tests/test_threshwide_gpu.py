"""EDR and LCSS at 5 .. 64 coordinates per point (csrc/threshwide.hip) against threshold_cases.py's host sweep, bit for bit."""
import numpy as np
import pytest

import pool_cases as pc
import seqdp_cases as sc
import threshold_cases as tc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS = 0.25
ref = pc.ref_cache()
MEASURES = [("edr", {}), ("edr", {"normalize": True}), ("lcss", {}), ("lcss", {"delta": 0}), ("lcss", {"delta": 5}), ("lcss", {"delta": 40})]


def proto_points(kinds, dim, rng, dtype=F32):
    """A prototype per entry of `kinds` (0, e_0, e_{dim//2}, e_{dim-1}, all ones) plus noise from {0, 0.25}, on the last coordinate
    from {0, 0.25, 0.5}: at eps 0.25 one prototype's points miss only at 0.5 apart there, others differ by >= 0.75 somewhere."""
    P = np.zeros((5, dim))
    P[1, 0] = P[2, dim // 2] = P[3, dim - 1] = 1.0
    P[4] = 1.0
    x = P[kinds] + 0.25 * rng.integers(0, 2, size=(len(kinds), dim))
    x[:, -1] = P[kinds, -1] + 0.25 * rng.integers(0, 3, size=len(kinds))
    return x.astype(dtype)


def proto_series(lengths, dim, seed, dtype=F32):
    rng = np.random.default_rng(seed)
    return [proto_points(rng.integers(0, 5, size=int(L)), dim, rng, dtype) for L in lengths]


def clustered_proto_series(nx, lo, hi, dim, seed, clusters=6):
    """Clusters: a member is a window of its cluster's sequence of prototypes with one in ten of them redrawn."""
    rng = np.random.default_rng(seed)
    base = np.random.default_rng(1000).integers(0, 5, size=(clusters, 2 * hi))

    def member(s):
        L = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, 2 * hi - L + 1))
        return proto_points(np.where(rng.random(L) < 0.1, rng.integers(0, 5, size=L), base[s % clusters, at:at + L]), dim, rng, F64)

    return [member(s) for s in range(nx)]


def check(key, name, kw, X, dtype):
    # (the key leaves dtype out: both dtypes hold the same values and share one reference)
    IJ = pc.all_ordered_pairs(len(X))
    want = ref((key, name, tuple(kw.items())), lambda: tc.HOSTS[name](X, IJ, EPS, **kw))
    got = pc.device_pairs(name, [x.astype(dtype) for x in X], IJ, eps=EPS, wide=True, **kw)
    assert np.array_equal(got, want)
    return got.reshape(len(X), len(X))


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("name, kw", MEASURES)
@pytest.mark.parametrize("dim", [5, 13, 64])
def test_word_and_strip_edges(dim, name, kw, dtype):
    """Lengths at the edges of 32-bit sweep words, 64-column blocks and 64-row strips; dim 5 and 13 are tail chunks, 64 four full
    ones; delta 0 is the diagonal alone, 5 lies inside a word, 40 crosses a word boundary either side of the diagonal."""
    X = proto_series([1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200], dim, seed=70 + dim)
    assert 0.1 < tc.match_share(X, EPS) < 0.25
    M = check(("edges", dim), name, kw, X, dtype)
    assert np.all(np.diag(M) == 0.0) and np.array_equal(M, M.T)
    if name == "lcss":
        assert np.any((M > 0.0) & (M < 1.0) & ~np.eye(len(X), dtype=bool))


@pytest.mark.parametrize("name, kw", [MEASURES[1], MEASURES[4]])
@pytest.mark.parametrize("dim, dtype", [(64, F32), (5, F64)])
def test_ceiling(dim, dtype, name, kw):
    check(("ceiling", dim), name, kw, proto_series([1024, 1023, 1], dim, seed=80 + dim), dtype)


def test_opt_in_and_limits():
    from annchor_amd import BruteForce, _native, distances

    X3 = tc.grid_series([1, 40, 130, 600], 3, seed=92)
    IJ = pc.all_ordered_pairs(len(X3))
    for name, kw in MEASURES:
        assert np.array_equal(pc.device_pairs(name, X3, IJ, eps=1.0, wide=True, **kw), pc.device_pairs(name, X3, IJ, eps=1.0, **kw))
    x, y = X5 = proto_series([10, 12], 5, seed=91, dtype=F64)
    for metric, kw in ((distances.EDR(EPS), None), ("edr", {"eps": EPS}), (distances.LCSS(EPS), None), ("lcss", {"eps": EPS})):
        with pytest.raises(ValueError, match="%s: series 0 has dim 5; dim 1 .. 4" % getattr(metric, "name", metric)):
            BruteForce(X5, metric, func_kwargs=kw)
    edr, lcss = distances.EDR(EPS, normalize=True, wide=True), distances.LCSS(EPS, delta=3, wide=True)
    assert edr(x, y) == tc.edr_loop(x, y, EPS, True) == edr(y, x) == edr.many([x], [y])[0] == edr.one_to_many(y, [x])[0]
    assert lcss(x, y) == tc.lcss_loop(x, y, EPS, 3) == lcss(y, x) == lcss.many([x], [y])[0] == lcss.one_to_many(y, [x])[0]
    v = np.random.default_rng(90).standard_normal((1025 + 10) * 5)
    bad = np.where(np.arange(v.size) == 3, np.nan, v)
    eng = _native.Engine(0)
    try:
        for setter, words in ((eng.set_edr_series_wide, "edr: the threshold eps"), (eng.set_lcss_series_wide, "lcss: the threshold eps")):
            for match, args, eps in [(r"error -4: .*dim 4.*5\.\.64", (v, [0, 10], [10, 10], 4), EPS),
                                     (r"error -4: .*dim 65.*5\.\.64", (np.zeros(20 * 65), [0, 10], [10, 10], 65), EPS),
                                     (r"error -4: .*1025.*1\.\.1024 at dim 5", (v, [0, 1025], [1025, 10], 5), EPS),
                                     (r"error -1: .*empty", (v, [0, 10], [10, 0], 5), EPS),
                                     ("error -1: .*non-finite", (bad, [0, 1024], [1024, 10], 5), EPS)] \
                    + [("error -1: " + words, (v, [0, 10], [10, 10], 5), e) for e in (np.nan, -1.0, np.inf)]:
                with pytest.raises(_native.NativeError, match=match):
                    setter(args[0], np.array(args[1]), np.array(args[2]), args[3], eps)
    finally:
        eng.close()


def test_edr_fit_brute_force_and_query():
    """test_editwide_gpu.py::test_erp_fit_brute_force_and_query under EDR at dim 13, which is no metric."""
    from annchor_amd import Annchor, BruteForce

    X, Q = clustered_proto_series(160, 20, 60, 13, seed=93), clustered_proto_series(20, 20, 60, 13, seed=94)
    nx, nall = len(X), len(X) + len(Q)
    T = pc.sym_matrix(lambda S, IJ: tc.edr_pairs_host(S, IJ, EPS), X + Q).ravel()
    kw = {"eps": EPS, "wide": True}

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(T[IJ[:, 0] * nall + IJ[:, 1]])

    def query_evaluator(f, Xs, Z, IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        rows = IJ[:, 0] if len(Xs) == nx else np.asarray(host_fit.A, dtype=np.int64)[IJ[:, 0]]
        return pairs(np.stack([rows, IJ[:, 1] + nx], axis=1))

    cfg = dict(func_kwargs=kw, is_metric=False, ols="lapack", **pc.FIT_CFG)
    host_fit = Annchor(X, "edr", get_exact_ijs=lambda f, Xs, IJ: pairs(IJ), **cfg).fit()
    dev = Annchor(X, "edr", **cfg).fit()
    assert dev.evals == host_fit.evals and all(np.array_equal(a, b) for a, b in zip(dev.neighbor_graph, host_fit.neighbor_graph))
    bf = BruteForce(X, "edr", func_kwargs=kw).fit()
    oi, od, _ = O.brute_force(pairs, nx)
    assert np.array_equal(bf.neighbor_graph[1], od) and np.array_equal(bf.neighbor_graph[0], oi)
    gi, gd = dev.query(Q, nn=5, p_work=0.3)
    hi, hd = host_fit.query(Q, nn=5, p_work=0.3, get_exact_query_ijs=query_evaluator)
    assert dev.query_evals == host_fit.query_evals and np.array_equal(gd, hd) and np.array_equal(gi, hi)


def test_rebinding():
    """One engine bound in turn gives a fresh engine's values: match_eps, edr_normalize, dtw_window and curve_dim do not leak."""
    from annchor_amd.utils import get_function_from_input

    lengths = [5, 90, 66, 1]
    eng = pc.bound("edr", proto_series([70, 3, 130], 5, seed=96), eps=EPS, normalize=True, wide=True)
    try:
        for name, X, kw in (("edr", tc.grid_series(lengths, 2, seed=97), {"eps": 1.0}),
                            ("lcss", proto_series(lengths, 6, seed=98), {"eps": EPS, "delta": 7, "wide": True}),
                            ("dtw", sc.one_of_each_length(lengths, 5, seed=99), {"wide": True})):
            IJ = pc.all_ordered_pairs(len(X))
            get_function_from_input(name, kw).bind(eng, X)
            assert np.array_equal(eng.metric_pairs(IJ), pc.device_pairs(name, X, IJ, **kw))
    finally:
        eng.close()
