"""The sequence measures on the device -- DTW, Frechet, ERP, MSM and TWE (csrc/seqdp.hip) and, in the sections whose body is the
same for strings, weighted Levenshtein (csrc/wed.hip) -- against the host recurrences of seqdp_cases.py and wed_cases.py.  One
test per section, parametrised over a spec per measure.  The two sections with many cases per measure (small and boundary
lengths) are bodies here that test_<measure>_gpu.py calls, beside the tests only that measure has.

Tolerance: none.  Every cell has fixed operands and min and max are exact, so every evaluation order gives the same bits; each
comparison of distances below is np.array_equal."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import dtw_cases as dc
import elastic_cases as lc
import erp_cases as ec
import frechet_cases as fc
import pool_cases as pc
import seqdp_cases as sc
import wed_cases as wc
from oracle import annchor_oracle as O

pytestmark = pytest.mark.gpu

ref = pc.ref_cache()   # (every key starts with the measure's name)
FIT_CFG = pc.FIT_CFG
NU, LAM = 0.37, 0.21   # TWE's non-default parameters
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------ the specs
# A measure's keyword parameters are spelt alike by its *_pairs_host, its *_loop, its class and func_kwargs, so one dict serves all.
def boundary_walks(measure, seed, flat=False):
    def build(dim):
        X = sc.one_of_each_length(sc.boundary_lengths(measure, dim), dim, seed=seed(dim), dtype=F32)
        return sc.univariate(X) if flat else X
    return build


def q_lengths_ok(Q):
    return min(map(len, Q)) >= 30 and max(map(len, Q)) <= 70 and len({len(q) for q in Q}) > 5


def fixed_length_query():
    """X is a 3-D array [240, 48, 2], Q a list of 20 members of 30..70 points."""
    X, Q = np.stack(sc.clustered_curves(240, 48, 48, 2, seed=33)), sc.clustered_curves(20, 30, 70, 2, seed=34)
    assert X.shape == (240, 48, 2) and q_lengths_ok(Q)
    return X, Q


def dtw_query():
    """X is an array (rows of 48 values), Q a list of 20 series of 30..70 values."""
    X, Q = np.stack(dc.clustered_series(240, 48, 48, seed=13)), dc.clustered_series(20, 30, 70, seed=14)
    assert X.shape == (240, 48) and q_lengths_ok(Q)
    return X, Q


def msm_query():
    """X is the fit data (240 series of 20..60 values), Q a list of 20 series of 30..70 values."""
    X, Q = lc.msm_fit_series(), sc.univariate(sc.clustered_curves(20, 30, 70, 1, seed=47))
    assert len(X) == 240 and q_lengths_ok(Q)
    return X, Q


def twe_query():
    """X is the fit data (240 series of dim 2, 20..60 points), Q a list of 20 series of 30..70 points."""
    X, Q = lc.twe_fit_series(), sc.clustered_curves(20, 30, 70, 2, seed=49)
    assert len(X) == 240 and q_lengths_ok(Q)
    return X, Q


def wed_query():
    """X is the fit data set (20..60 symbols); Q holds an empty string, a string of 2048 symbols and 18 strings of 5..90 symbols:
    the engine that holds X and Q runs the widest shape."""
    Q = ["", wc.one_of_each_length([2048], wc.FIT_A, seed=34)[0]] + wc.clustered_strings(18, 5, 90, wc.FIT_A, seed=35, edits=0.6)
    assert len(Q) == 20 and len({len(q) for q in Q}) > 8
    return wc.fit_strings(), Q


def points_of_dim_3(X):
    return all(x.shape[1] == 3 for x in X)


def flat_members(X):
    return all(x.ndim == 1 for x in X)


def raises_value_error(match, X, name, **kw):
    from annchor_amd import BruteForce

    with pytest.raises(ValueError, match=match):
        BruteForce(X, name, **kw)


def dtw_limits(rng):
    """-> the host's refusals (match, members, BruteForce's keywords), the class's (match, keywords), the library's own behind
    them (match, call on an engine), and what the library must take (call on an engine -> bool)."""
    from annchor_amd import BruteForce

    v = rng.standard_normal(2049 + 10)
    bad = v.copy()
    bad[3] = np.nan
    return ([("2049", [rng.standard_normal(2049), rng.standard_normal(10)], {})], [],
            [("error -4", lambda eng: BruteForce([rng.standard_normal(10)], "dtw")),
             (r"error -4: .*2049.*1\.\.2048", lambda eng: eng.set_series(v, np.array([0, 2049]), np.array([2049, 10]))),
             ("error -1: .*non-finite", lambda eng: eng.set_series(bad, np.array([0, 2048]), np.array([2048, 10])))], [])


def frechet_limits(rng):
    v, v3 = rng.standard_normal((2049 + 10) * 2), rng.standard_normal((1025 + 10) * 3)
    bad = v.copy()
    bad[3] = np.nan
    return ([("curve 0 has 2049 points", [rng.standard_normal((2049, 2)), rng.standard_normal((10, 2))], {}),
             ("curve 1 has 1025 points", [rng.standard_normal((10, 3)), rng.standard_normal((1025, 3))], {}),
             ("curve 0 has dim 5", [rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], {}),
             ("curve 1 has dim 3, curve 0 has dim 2", [rng.standard_normal((10, 2)), rng.standard_normal((10, 3))], {})], [],
            [(r"error -4: .*2049.*1\.\.2048", lambda eng: eng.set_curves(v, np.array([0, 2049]), np.array([2049, 10]), 2)),
             (r"error -4: .*1025.*1\.\.1024", lambda eng: eng.set_curves(v3, np.array([0, 1025]), np.array([1025, 10]), 3)),
             (r"error -4: .*dim 5", lambda eng: eng.set_curves(v, np.array([0, 10]), np.array([10, 10]), 5)),
             (r"error -1: .*empty", lambda eng: eng.set_curves(v, np.array([0, 10]), np.array([10, 0]), 2)),
             ("error -1: .*non-finite", lambda eng: eng.set_curves(bad, np.array([0, 2048]), np.array([2048, 10]), 2))], [])


def series_limits(name, rng, L1, L2):
    """The refusals ERP and TWE word alike: lengths past the limit at dim 1 and 2, dims, an empty member, a value that is not
    finite; on the host and from the engine's set_<name>_series."""
    v1, v = rng.standard_normal(L1 + 1 + 10), rng.standard_normal((L2 + 1 + 10) * 2)
    bad = v.copy()
    bad[3] = np.nan

    def setter(*args):
        return lambda eng: getattr(eng, "set_%s_series" % name)(*args)

    return ([("%s: series 0 has %d points" % (name, L1 + 1), [rng.standard_normal(L1 + 1), rng.standard_normal(10)], {}),
             ("%s: series 1 has %d points" % (name, L2 + 1), [rng.standard_normal((10, 2)), rng.standard_normal((L2 + 1, 2))], {}),
             ("%s: series 0 has dim 5" % name, [rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], {}),
             ("%s: series 1 has dim 3, series 0 has dim 2" % name, [rng.standard_normal((10, 2)), rng.standard_normal((10, 3))], {}),
             ("%s: series 1 is empty" % name, [rng.standard_normal((10, 2)), np.zeros((0, 2))], {}),
             ("%s: series 0 .*not finite" % name, [np.array([1.0, np.nan]), rng.standard_normal(10)], {})],
            [(r"error -4: .*%d.*1\.\.%d at dim 1" % (L1 + 1, L1), setter(v1, np.array([0, L1 + 1]), np.array([L1 + 1, 10]), 1)),
             (r"error -4: .*%d.*1\.\.%d at dim 2" % (L2 + 1, L2), setter(v, np.array([0, L2 + 1]), np.array([L2 + 1, 10]), 2)),
             (r"error -4: .*dim 5", setter(v, np.array([0, 10]), np.array([10, 10]), 5)),
             (r"error -1: .*empty", setter(v, np.array([0, 10]), np.array([10, 0]), 2)),
             ("error -1: .*non-finite", setter(bad, np.array([0, L2]), np.array([L2, 10]), 2))], v, setter)


def erp_limits(rng):
    host, native, v, setter = series_limits("erp", rng, 2048, 1024)
    gap = "erp: gap must be a finite real number"
    host.append((gap, [rng.standard_normal(10), rng.standard_normal(10)], {"func_kwargs": {"gap": np.nan}}))
    native[4:4] = [(r"error -1: .*gap", setter(v, np.array([0, 10]), np.array([10, 10]), 2, g)) for g in (np.nan, np.inf)]
    return host, [(gap, {"gap": np.nan})], native, []


def twe_limits(rng):
    host, native, v, setter = series_limits("twe", rng, sc.max_length("twe", 1), sc.max_length("twe", 2))
    host.append(("twe: lam must be a finite real number >= 0", [rng.standard_normal(10), rng.standard_normal(10)],
                 {"func_kwargs": {"lam": np.nan}}))
    for bad in (np.nan, np.inf, -0.5):
        native[4:4] = [(r"error -1: twe: the stiffness nu", setter(v, np.array([0, 10]), np.array([10, 10]), 2, bad, 1.0)),
                       (r"error -1: twe: the penalty lam", setter(v, np.array([0, 10]), np.array([10, 10]), 2, 0.001, bad))]
    return host, [("twe: nu must be a finite real number >= 0", {"nu": -1.0})], native, []


def msm_limits(rng):
    LIMIT = sc.max_length("msm", 1)
    v, w = rng.standard_normal(LIMIT + 1 + 10), rng.standard_normal(LIMIT + 10)
    bad = v.copy()
    bad[3] = np.nan
    c = "msm: c must be a finite real number > 0"

    def limit_taken(eng):
        eng.set_msm_series(w, np.array([0, LIMIT]), np.array([LIMIT, 10]), 1.0)
        return eng.metric_pairs(np.array([[0, 1]]))[0] == sc.msm_pairs_host([w[:LIMIT], w[LIMIT:]], [[0, 1]])[0]

    return ([("msm: series 0 has 2049 values", [rng.standard_normal(LIMIT + 1), rng.standard_normal(10)], {}),
             ("msm: series 1 has 2 dimensions; univariate", [rng.standard_normal(10), rng.standard_normal((10, 2))], {}),
             ("msm: series 0 has 2 dimensions; univariate", [rng.standard_normal((10, 5)), rng.standard_normal((10, 5))], {}),
             ("msm: series 1 is empty", [rng.standard_normal(10), np.zeros(0)], {}),
             ("msm: series 0 .*not finite", [np.array([1.0, np.nan]), rng.standard_normal(10)], {}),
             (c, [rng.standard_normal(10), rng.standard_normal(10)], {"func_kwargs": {"c": np.nan}})], [(c, {"c": 0.0})],
            [(r"error -4: .*series 0 has 2049 values.*1\.\.2048",
              lambda eng: eng.set_msm_series(v, np.array([0, LIMIT + 1]), np.array([LIMIT + 1, 10]), 1.0)),
             (r"error -1: .*series 1 is empty", lambda eng: eng.set_msm_series(v, np.array([0, 10]), np.array([10, 0]), 1.0))]
            + [(r"error -1: msm: the cost c", lambda eng, b=b: eng.set_msm_series(v, np.array([0, 10]), np.array([10, 10]), b))
               for b in (np.nan, np.inf, 0.0, -1.0)]
            + [("error -1: .*series 0 holds a non-finite",
                lambda eng: eng.set_msm_series(bad, np.array([0, 1024]), np.array([1024, 10]), 1.0))], [limit_taken])


def spec(name, host, **fields):
    """host(X, IJ, **parameters) is the measure's *_pairs_host.  kw: what func_kwargs holds in the fit, brute-force and query
    sections (the defaults, except for the cost table of weighted Levenshtein).  The other fields default to "has no such section"."""
    s = SimpleNamespace(name=name, host=host, kw={}, ann_kw={}, is_metric=True, no_ties=False, query_fit_from_ref=False, loop=None,
                        params=[], limits=None)
    s.__dict__.update(fields)
    return s


WED_KW = wc.kwargs_of(wc.fit_costs())
SPECS = [
    spec("dtw", sc.dtw_pairs_host, is_metric=False, ann_kw={"is_metric": False},
         fit=dc.fit_series, brute=dc.brute_series, brute_check=flat_members, query=dtw_query, limits=dtw_limits),
    spec("frechet", sc.frechet_pairs_host, loop=fc.frechet_loop, cls="Frechet", loose_dim=3, loose_flat=True,
         boundary=boundary_walks("frechet", lambda dim: 50 + dim), boundary_kw={},
         fit=fc.fit_curves, brute=fc.brute_curves, brute_check=points_of_dim_3, query=fixed_length_query, limits=frechet_limits),
    spec("erp", sc.erp_pairs_host, loop=ec.erp_loop, cls="ERP", loose_dim=3, loose_flat=True, loose_kw={"gap": 1.0},
         known=[([3.0], [1.0, 1.0], {"gap": 1.0}, 2.0), ([3.0], [1.0, 1.0], {}, 3.0)],
         boundary=boundary_walks("erp", lambda dim: 50 + dim), boundary_kw={"gap": 0.37},
         fit=ec.fit_curves, brute=ec.brute_curves, brute_check=points_of_dim_3, query=fixed_length_query,
         params=[{"gap": 0.5}], param_data=ec.univariate_series, param_stride=5, limits=erp_limits),
    spec("msm", sc.msm_pairs_host, loop=lc.msm_loop, cls="MSM", loose_dim=None, loose_flat=False, loose_kw={"c": 0.25}, no_ties=True,
         known=[([1, 2, 3], [2, 2, 2], {"c": 0.5}, 2.0), ([0], [4], {"c": 1.0}, 4.0), ([1, 1, 1, 5], [1, 5], {"c": 0.25}, 0.5),
                ([3, 1, 4, 1, 5], [2, 7, 1], {"c": 1.0}, 11.0)],
         boundary=boundary_walks("msm", lambda dim: 50, flat=True), boundary_kw={"c": 0.37},
         fit=lc.msm_fit_series, brute=lc.msm_brute_series, brute_check=flat_members, query=msm_query,
         params=[{"c": 0.25}], param_data=lc.msm_fit_series, param_stride=11, limits=msm_limits),
    spec("twe", sc.twe_pairs_host, loop=lc.twe_loop, cls="TWE", loose_dim=3, loose_flat=True, loose_kw={"nu": NU, "lam": LAM},
         no_ties=True,
         known=[([1, 2, 3], [2, 2, 2], {"nu": 0.25, "lam": 0.5}, 3.0), ([0], [4], {"nu": 0.5, "lam": 1.0}, 4.0),
                ([1, 1, 1, 5], [1, 5], {"nu": 0.125, "lam": 0.5}, 1.75), ([3, 1, 4, 1, 5], [2, 7, 1], {"nu": 0.5, "lam": 1.0}, 19.0)],
         boundary=boundary_walks("twe", lambda dim: 50 + dim), boundary_kw={"nu": NU, "lam": LAM},
         fit=lc.twe_fit_series, brute=lc.twe_brute_series, brute_check=points_of_dim_3, query=twe_query,
         params=[{"nu": NU, "lam": LAM}, {"nu": 0.0, "lam": 0.5}], param_data=lc.twe_univariate_series, param_stride=5,
         limits=twe_limits),
    spec("weighted_levenshtein", lambda X, IJ: wc.wed_pairs_host(X, IJ, wc.fit_costs()), kw=WED_KW, ann_kw={"func_kwargs": WED_KW},
         fit=wc.fit_strings, brute=wc.brute_strings, brute_check=lambda X: min(map(len, X)) >= 20 and max(map(len, X)) <= 60,
         query=wed_query, query_fit_from_ref=True),
]
BY_NAME = {s.name: s for s in SPECS}


def per(cases):
    """One parameter per (spec, case) of cases(spec), named <measure>-<case>."""
    return [pytest.param(s, c, id="%s-%s" % (s.name, tag)) for s in SPECS for tag, c in cases(s)]


every = pytest.mark.parametrize("s", SPECS, ids=lambda s: s.name)


def fit_ref(s):
    """Every pair of the measure's fit data set, [nx * nx]."""
    return ref((s.name, "fit"), lambda: pc.sym_matrix(s.host, s.fit()).ravel())


def fit_pairs(s):
    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(fit_ref(s)[IJ[:, 0] * len(s.fit()) + IJ[:, 1]])
    return pairs


def func_kwargs(kw):
    return {"func_kwargs": kw} if kw else {}


# ------------------------------------------------------------------------------------ 1, 2. small and boundary lengths
# These two sections have many cases per measure, so their tests stay where they were -- test_<measure>_gpu.py, one thin test
# each, beside the tests only that measure has -- and call the bodies here; the cache of references is this module's.
def small_lengths(s, X, tag, **kw):
    """One member of each length 1..longest, all ordered pairs: n < m, n > m, n = m, length 1 against everything, every strip and
    group boundary of the 4-pairs-per-wavefront shape; then the list without its last 3 pairs (a last wavefront with one pair
    in it).  tag: what tells this data set from the measure's others."""
    IJ = pc.all_ordered_pairs(len(X))
    want = ref((s.name, "small") + tuple(tag), lambda: s.host(X, IJ, **kw))
    assert np.all(np.isfinite(want))
    eng = pc.bound(s.name, X, **kw)
    got, got_part = eng.metric_pairs(IJ), eng.metric_pairs(IJ[:-3])
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got_part, want[:-3])
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T)


def boundary_lengths(s, dim, shape, dtype):
    """The strip and group boundaries {R-1, R, R+1, 2R, GR-1, GR, GR+1} of every shape (R, G) at this dim, the limit (the
    package's) and the limit minus 1, on the shape of each capacity; non-default parameters (ERP: both prefix boundaries carry
    values of their own).  One float32 random walk per length: the float64 data set is the same values widened, so both share
    a reference."""
    limit = sc.max_length(s.name, dim)
    Ls = sc.boundary_lengths(s.name, dim)
    R, G = sc.instantiations(s.name, dim)[shape]
    assert {7, 8, 9, 16, 127, 128, 129, 511, 512, 513, limit - 1, limit} <= set(Ls)
    assert {R - 1, R, R + 1, 2 * R, G * R - 1, G * R} <= set(Ls)
    X = s.boundary(dim)
    nkeep, IJ = sc.boundary_case(s.name, dim, shape)
    sub = X[:nkeep]
    want = ref((s.name, "boundary", dim, shape), lambda: s.host(sub, IJ, **s.boundary_kw))
    assert np.all(np.isfinite(want))
    got = pc.device_pairs(s.name, [x.astype(dtype) for x in sub], IJ, **s.boundary_kw)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------------------------- 3. PairSource forms
@every
def test_pair_source_forms(s):
    """Explicit pairs (metric_pairs), one-to-all (the anchor rows of a fit: ann.D), and positions into the pair list with the
    result written to RefineApprox / not_computed_mask (the sampling and refinement stages of a fit)."""
    from annchor_amd import Annchor, _native

    X = s.fit()
    X[7] = copy.copy(X[3])          # identical members
    nx = len(X)
    IJ = pc.all_ordered_pairs(nx)[::7]
    want = s.host(X, IJ)
    eng = pc.bound(s.name, X, **s.kw)
    got = eng.metric_pairs(IJ)
    assert np.array_equal(got, want)
    assert eng.metric_pairs(np.array([[3, 7], [7, 3], [5, 5]])).tolist() == [0.0, 0.0, 0.0]
    eng.pick_anchors_selected([3, 100])
    D = eng.download(_native.F_D).reshape(nx, 2)
    eng.close()
    for col, a in enumerate((3, 100)):
        assert np.array_equal(D[:, col], s.host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    assert D[7, 0] == 0.0 and D[3, 0] == 0.0
    ann = Annchor(X, s.name, **s.ann_kw, **FIT_CFG).fit()
    A = np.asarray(ann.A)
    for col, a in enumerate(A):
        assert np.array_equal(ann.D[:, col], s.host(X, np.stack([np.full(nx, a), np.arange(nx)], 1)))
    done = ~ann.not_computed_mask
    assert done.sum() >= ann.evals - ann.n_anchors * nx > 0
    assert np.array_equal(ann.RefineApprox[done], s.host(X, ann.IJs[done]))


@pytest.mark.parametrize("s, kw", per(lambda s: [("-".join("%s%s" % kv for kv in kw.items()), kw) for kw in s.params]))
def test_parameters_reach_the_kernel(s, kw):
    """A second engine with other parameters, through explicit pairs, one-to-all and a fit: the values differ from the defaults',
    and equal the host's (ERP: cell costs and both prefix boundaries; TWE: nu = 0 is one case)."""
    from annchor_amd import Annchor, _native

    X = s.param_data()
    nx = len(X)
    IJ = pc.all_ordered_pairs(nx)[::s.param_stride]
    want = s.host(X, IJ, **kw)
    want0 = ref((s.name, "defaults"), lambda: s.host(X, IJ))
    assert not np.array_equal(want, want0)
    eng0, eng = pc.bound(s.name, X), pc.bound(s.name, X, **kw)
    got0, got = eng0.metric_pairs(IJ), eng.metric_pairs(IJ)
    eng.pick_anchors_selected([11])
    D = eng.download(_native.F_D).reshape(nx)
    eng0.close()
    eng.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got0, want0)
    assert np.array_equal(D, s.host(X, np.stack([np.full(nx, 11), np.arange(nx)], 1), **kw))
    ann = Annchor(X, s.name, func_kwargs=kw, **FIT_CFG).fit()
    idx, dist = ann.neighbor_graph
    NN = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), s.host(X, NN, **kw))


# ------------------------------------------------------------------------------------------------------ 4. BruteForce
@every
def test_brute_force(s):
    from annchor_amd import BruteForce

    X = s.brute()
    assert len(X) == 200 and s.brute_check(X) and len({len(x) for x in X}) > 20
    bf = BruteForce(X, s.name, **func_kwargs(s.kw)).fit()
    nx = len(X)
    T = pc.sym_matrix(s.host, X)
    oi, od, _ = O.brute_force(lambda IJ: T[IJ[:, 0], IJ[:, 1]], nx)
    assert np.array_equal(bf.neighbor_graph[1], od)
    assert np.array_equal(bf.neighbor_graph[0], oi)


# ---------------------------------------------------------------------------------------------------------- 5. fits
@every
def test_fit_parity_with_the_cpu_pipeline(s, capsys):
    """A measure that is no metric (DTW) is fitted with is_metric left at True: the constructor warns, and the pipeline is the
    oracle's all the same; its default-solver fit is test_dtw_gpu.py::test_fit_without_the_triangle_inequality."""
    from annchor_amd import Annchor, compare_neighbor_graphs

    X = s.fit()
    nx = len(X)
    if s.no_ties:
        off = fit_ref(s).reshape(nx, nx)[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
        assert all(len(np.unique(row)) == nx - 1 for row in off)   # no ties within a row: the index comparisons rest on no tie rule
    ann = Annchor(X, s.name, ols="lapack", **func_kwargs(s.kw), **FIT_CFG)
    assert ("triangle inequality" in capsys.readouterr().err) == (not s.is_metric)
    ann.fit()
    ora = O.OracleAnnchor(nx, fit_pairs(s), **FIT_CFG).fit()
    assert np.array_equal(ann.A, ora.A)
    assert np.array_equal(ann.D, ora.D)
    assert ann.evals == ora.evals
    assert np.array_equal(ann.neighbor_graph[1], ora.neighbor_graph[1])
    assert np.array_equal(ann.neighbor_graph[0], ora.neighbor_graph[0])
    if not s.is_metric:
        return
    # the default solver: whatever the graph lists is an exact distance
    dflt = Annchor(X, s.name, **func_kwargs(s.kw), **FIT_CFG).fit()
    assert "triangle inequality" not in capsys.readouterr().err
    idx, dist = dflt.neighbor_graph
    IJ = np.stack([np.repeat(np.arange(nx), idx.shape[1]), np.asarray(idx).ravel()], axis=1)
    assert np.array_equal(np.asarray(dist).ravel(), fit_pairs(s)(IJ))
    # (recorded in DESIGN.md, not asserted: wrong neighbours against the exact graph)
    exact = O.brute_force(fit_pairs(s), nx)
    k = FIT_CFG["n_neighbors"]
    print("%s is_metric=True, p_work=0.3: %d evaluations, %d of %d neighbours differ from the exact graph"
          % (s.name, dflt.evals, compare_neighbor_graphs(exact[:2], dflt.neighbor_graph, k), nx * k))


# ----------------------------------------------------------------------------------------------------------- 6. query
@every
def test_query_with_other_lengths(s):
    """The data sets are the docstrings of the specs' query builders."""
    from annchor_amd import Annchor

    X, Q = s.query()
    both = list(X) + Q
    nx = len(X)
    ann = Annchor(X, s.name, ols="lapack", **func_kwargs(s.kw), **FIT_CFG).fit()
    gi, gd = ann.query(Q, nn=5, p_work=0.3)
    ora = O.OracleAnnchor(nx, fit_pairs(s) if s.query_fit_from_ref else lambda IJ: s.host(both, IJ), **FIT_CFG).fit()
    oi, od, info = O.query(ora, lambda IJ: s.host(both, np.stack([IJ[:, 0], IJ[:, 1] + nx], 1)), len(Q), nn=5, p_work=0.3)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gd, od)
    assert np.array_equal(gi, oi)


# --------------------------------------------------------------------------------------------------- 7. loose objects
@pytest.mark.parametrize("s", [s for s in SPECS if s.loop], ids=lambda s: s.name)
def test_loose_objects(s):
    from annchor_amd import distances

    cls, f, loop = getattr(distances, s.cls), getattr(distances, s.name), s.loop
    rng = np.random.default_rng(6)
    size = (lambda L: L) if s.loose_dim is None else (lambda L: (L, s.loose_dim))
    xs = [np.cumsum(rng.standard_normal(size(L)), axis=0) for L in (5, 40, 1, 130)]
    ys = [np.cumsum(rng.standard_normal(size(L)), axis=0) for L in (17, 9, 33, 2)]
    assert f(xs[0], ys[0]) == loop(xs[0], ys[0])
    assert f(ys[1], xs[1]) == loop(ys[1], xs[1])
    assert np.array_equal(f.many(xs, ys), [loop(x, y) for x, y in zip(xs, ys)])
    assert np.array_equal(f.one_to_many(xs[1], ys), [loop(xs[1], y) for y in ys])
    a, b = xs[0], ys[0]
    if s.loose_flat:   # univariate members
        a, b = rng.standard_normal(12), rng.standard_normal(7)
        assert f(a, b) == loop(a, b)
    # the known answers
    for x, y, kw, want in getattr(s, "known", []):
        assert cls(**kw)(np.array(x, dtype=F64), np.array(y, dtype=F64)) == want
        assert cls(**kw)(np.array(y, dtype=F32), np.array(x, dtype=F32)) == want
    # parameters of its own
    kw = getattr(s, "loose_kw", None)
    if kw:
        g = cls(**kw)
        assert g(a, b) == loop(a, b, **kw) != f(a, b)
        assert np.array_equal(g.many(xs, ys), [loop(x, y, **kw) for x, y in zip(xs, ys)])


# ---------------------------------------------------------------------------------------------------------- 8. limits
@pytest.mark.parametrize("s", [s for s in SPECS if s.limits], ids=lambda s: s.name)
def test_limits(s):
    from annchor_amd import _native, distances

    host, own, native, taken = s.limits(np.random.default_rng(5))
    for match, X, kw in host:
        raises_value_error(match, X, s.name, **kw)
    for match, kw in own:
        with pytest.raises(ValueError, match=match):
            getattr(distances, s.cls)(**kw)
    # the library's own checks, behind the host's
    eng = _native.Engine(0)
    try:
        for match, call in native:
            with pytest.raises(_native.NativeError, match=match):
                call(eng)
        for call in taken:   # the limit itself is taken
            assert call(eng)
    finally:
        eng.close()
