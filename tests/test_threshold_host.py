"""EDR and LCSS on the host: seqdp_cases.py's sweep and its lane-by-lane restatement of the kernel's schedule (csrc/seqdp.hip)
with the two threshold measures against the plain double loops, the known answers, two cross-checks against measures the
project already pins (unit Levenshtein, weighted Levenshtein), the packers, parameter refusals, the name lookup, the is-metric
note and the usability of the fit data.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import pool_cases as pc
import seqdp_cases as sc
import threshold_cases as tc
import wed_cases as wc
from oracle import annchor_oracle as O
from oracle import metrics as om

EDR_KW = [{"normalize": False}, {"normalize": True}]
LCSS_KW = [{"delta": None}, {"delta": 0}, {"delta": 5}]


def mixed_series(dim, seed):
    """Grid series (differences of exactly eps) of lengths 1..12 and a few up to 70, some of them float32."""
    lengths = list(range(1, 13)) + [31, 47, 70]
    return tc.grid_series(lengths, dim, seed) + tc.grid_series(lengths[::3], dim, seed + 1, dtype=np.float32)


# ------------------------------------------------------------------------------------------ 1. loop == sweep == lanes
@pytest.mark.parametrize("dim", sc.DIMS)
def test_sweep_equals_the_double_loops(dim):
    """All ordered pairs (both argument orders), bit for bit; symmetric, zero on the diagonal, LCSS within [0, 1]."""
    X = mixed_series(dim, 10 + dim)
    eps = tc.GRID_EPS[dim]
    assert 0.2 <= tc.match_share(X, eps) <= 0.8
    IJ = pc.all_ordered_pairs(len(X))
    for kw in EDR_KW:
        got = tc.edr_pairs_host(X, IJ, eps, **kw)
        assert np.array_equal(got, [tc.edr_loop(X[i], X[j], eps, **kw) for i, j in IJ])
        assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T) and np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    for kw in LCSS_KW:
        got = tc.lcss_pairs_host(X, IJ, eps, **kw)
        assert np.array_equal(got, [tc.lcss_loop(X[i], X[j], eps, **kw) for i, j in IJ])
        assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T) and np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
        assert got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", sc.DIMS)
@pytest.mark.parametrize("measure", ["edr", "lcss"])
def test_lane_by_lane_restatement_equals_the_double_loop(measure, dim, shape):
    """The schedule of k_seqdp<T, DIM, R, G, EdrOp / LcssOp> on 64 lanes -- EDR's counted edges (column -1 of a lane's rows, its
    bottom cell, lane 0's row -1 riding the strip) and LCSS's zeros, and the delta test on e = l R + r - jc -- against the loops,
    on seqdp_cases.lane_case.  At the widest shape the double loop runs on the pairs with a short partner, the long pairs go
    through the sweep the test above ties to it."""
    R, G = sc.instantiations(measure, dim)[shape]
    Ls, IJ = sc.lane_case(measure, dim, shape)
    X = tc.grid_series(Ls, dim, seed=70 + 10 * dim + shape)
    eps = tc.GRID_EPS[dim]
    if measure == "edr":
        kw = {"normalize": shape == 1}
        got, want, loop = tc.edr_lanes(X, IJ, eps, kw["normalize"], R, G), tc.edr_pairs_host(X, IJ, eps, **kw), tc.edr_loop
    else:
        kw = {"delta": (None, 0, 5)[shape]}
        got, want, loop = tc.lcss_lanes(X, IJ, eps, kw["delta"], R, G), tc.lcss_pairs_host(X, IJ, eps, **kw), tc.lcss_loop
    check = np.flatnonzero((IJ < 2).any(axis=1)) if shape == 2 else np.arange(len(IJ))
    assert np.array_equal(want[check], [loop(X[i], X[j], eps, **kw) for i, j in IJ[check]])
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------- 2. known answers
def test_known_answers():
    f = np.float64
    for a, b in (([0, 0, 0], [5]), ([5], [0, 0, 0])):
        assert tc.edr_loop(f(a), f(b), 1.0) == 3.0 == tc.edr_pairs_host([f(a), f(b)], [[0, 1]], 1.0)[0]
    assert tc.edr_loop(f([1, 2, 3]), f([1, 2, 3]), 0.0) == 0.0
    x, y = f([1, 2, 3, 4]), f([1.4, 3.5, 9])
    assert abs(3.0 - 3.5) == 0.5                                    # the 3.5 sits at a difference of exactly eps
    assert tc.edr_loop(x, y, 0.5) == 2.0 == tc.edr_loop(y, x, 0.5) == tc.edr_pairs_host([x, y], [[0, 1]], 0.5)[0]
    assert tc.edr_loop(x, y, np.nextafter(0.5, 0.0)) == 3.0         # what `<` in place of `<=` would give
    assert tc.edr_loop(x, y, 0.5, normalize=True) == 0.5
    x, y = f([1, 2, 3, 4]), f([2, 4])
    assert tc.lcss_count_loop(x, y, 0.0) == 2.0 and tc.lcss_loop(x, y, 0.0) == 0.0 == tc.lcss_pairs_host([x, y], [[1, 0]], 0.0)[0]
    assert tc.lcss_count_loop(x, y, 0.0, delta=0) == 0.0 and tc.lcss_loop(x, y, 0.0, delta=0) == 1.0
    assert tc.lcss_pairs_host([x, y], [[0, 1], [1, 0]], 0.0, delta=0).tolist() == [1.0, 1.0]
    x, y = f([1, 2, 3, 4]), f([4, 1, 2])
    assert tc.lcss_count_loop(x, y, 0.0, delta=1) == 2.0
    assert tc.lcss_loop(x, y, 0.0, delta=1) == 1.0 - 2.0 / 3.0 == tc.lcss_pairs_host([x, y], [[0, 1]], 0.0, delta=1)[0]


# --------------------------------------------------------------------------------------------------- 3. cross-checks
def test_edr_and_lcss_against_the_string_measures():
    """At dim 1 and eps = 0 on integer-valued series, EDR is the unit Levenshtein distance of the sequences read as strings, and
    n + m - 2 L of LCSS without delta is the weighted Levenshtein distance with substitution cost 2 and indel cost 1."""
    X = tc.integer_sequences()
    assert len(X) == 60 and min(map(len, X)) >= 1 and max(map(len, X)) <= 40
    strings = ["".join(wc.SYMBOLS[int(v)] for v in x) for x in X]
    IJ = pc.all_ordered_pairs(len(X))
    n, m = tc._lens(X, IJ)
    edr = tc.edr_pairs_host(X, IJ, 0.0)
    assert np.array_equal(edr, [om.levenshtein(strings[i], strings[j], algo="dp") for i, j in IJ])
    count = sc.pairs_host(X, IJ, tc.Lcss(0.0))
    costs = wc.Costs(wc.SYMBOLS[:4], 2.0 * (1.0 - np.eye(4)), np.ones(4))
    assert np.array_equal(n + m - 2.0 * count, wc.wed_pairs_host(strings, IJ, costs))


# ------------------------------------------------------------------------------- 4. packers, parameters, name lookup
def test_packers_and_limits():
    from annchor_amd import distances as d

    assert d.EDR_MAX_DIM == d.LCSS_MAX_DIM == d.DTW_MAX_DIM == 4
    for dim in sc.DIMS:
        want = 2048 if dim <= 2 else 1024
        assert d.edr_max_length(dim) == d.lcss_max_length(dim) == d.dtw_max_length(dim) == want
        assert sc.max_length("edr", dim) == sc.max_length("lcss", dim) == sc.max_length("dtw", dim) == want
    assert d.dtw_max_length(1) == d.DTW_MAX_LENGTH
    rng = np.random.default_rng(3)
    cur = [rng.standard_normal((L, 3)) for L in (1, 5, 1024, 17)]
    for pack in (d.pack_edr_series, d.pack_lcss_series, d.pack_dtw_series):
        values, offs, lens, dim = pack(cur)
        assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32 and dim == 3
        assert list(lens) == [1, 5, 1024, 17] and list(offs) == [0, 1, 6, 1030]
        assert np.array_equal(values, np.concatenate([c.ravel() for c in cur]))
        assert pack([c.astype(np.float32) for c in cur])[0].dtype == np.float32
        assert pack([rng.standard_normal(4), rng.standard_normal(2048)])[3] == 1


@pytest.mark.parametrize("name", ["edr", "lcss", "dtw"])
def test_packers_refuse(name):
    from annchor_amd import distances as d

    pack = getattr(d, "pack_%s_series" % name)
    for bad, match in [([np.ones(2049), np.ones(3)], "%s: series 0 has 2049 points; at most 2048 are supported at dim 1" % name),
                       ([np.ones((3, 3)), np.ones((1025, 3))], "%s: series 1 has 1025 points; at most 1024 are supported at dim 3" % name),
                       ([np.ones((3, 5)), np.ones((3, 5))], "%s: series 0 has dim 5; dim 1 .. 4" % name),
                       ([np.ones((3, 2)), np.ones((3, 3))], "%s: series 1 has dim 3, series 0 has dim 2" % name),
                       ([np.ones((3, 2)), np.zeros((0, 2))], "%s: series 1 is empty" % name),
                       ([np.ones((3, 2)), np.full((3, 2), np.inf)], "%s: series 1 .*not finite" % name),
                       ([np.ones((3, 2, 2)), np.ones(3)], "%s: series 0 has 3 dimensions" % name)]:
        with pytest.raises(ValueError, match=match):
            pack(bad)


@pytest.mark.parametrize("eps", [np.nan, np.inf, -np.inf, -0.5, "0.5", None, 1j, True])
def test_eps_must_be_a_finite_number_not_below_zero(eps):
    from annchor_amd.distances import EDR, LCSS

    with pytest.raises(ValueError, match="edr: eps must be a finite real number >= 0"):
        EDR(eps)
    with pytest.raises(ValueError, match="lcss: eps must be a finite real number >= 0"):
        LCSS(eps)


def test_other_parameters():
    from annchor_amd.distances import EDR, LCSS

    assert EDR(0).eps == 0.0 and EDR(np.float32(0.5)).eps == 0.5 and EDR(1, normalize=True).normalize is True
    assert LCSS(0.5).delta is None and LCSS(0.5, delta=np.int64(3)).delta == 3 and LCSS(0.5, delta=0).delta == 0
    for delta in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="lcss: delta must be None or an integer >= 0"):
            LCSS(0.5, delta=delta)
    for normalize in (1, None, "yes"):
        with pytest.raises(ValueError, match="edr: normalize must be True or False"):
            EDR(0.5, normalize=normalize)
    with pytest.raises(TypeError):
        EDR()   # eps has no default


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("edr", {"eps": 0.25})
    assert isinstance(f, distances.EDR) and isinstance(f, distances.DeviceMetric) and f.name == "edr" and f.ragged
    assert f.eps == 0.25 and f.normalize is False
    assert get_function_from_input("edr", {"eps": 1, "normalize": True}).normalize is True
    g = get_function_from_input("lcss", {"eps": 0.25})
    assert isinstance(g, distances.LCSS) and g.name == "lcss" and g.ragged and g.eps == 0.25 and g.delta is None
    assert get_function_from_input("lcss", {"eps": 0.25, "delta": 5}).delta == 5
    for name in ("edr", "lcss"):
        for kw in (None, {}, {"delta": 3}):
            with pytest.raises(AssertionError, match="%s metric requires eps kwarg" % name):
                get_function_from_input(name, kw)
        with pytest.raises(ValueError, match="finite real number"):
            get_function_from_input(name, {"eps": np.nan})


# ------------------------------------------------------------------------------------------- 5. the fit data is usable
@pytest.mark.parametrize("name, kw", [(n, kw) for n in ("edr", "lcss") for kw in tc.FIT_PARAMS[n]],
                         ids=lambda v: v if isinstance(v, str) else "-".join("%s%s" % kv for kv in v.items()))
def test_fit_data_is_usable(name, kw):
    """The GPU fit tests' data set and configurations pass the CPU restatement of the pipeline: the stratified sampler finds
    enough samples in every bin (LCSS and normalised EDR saturate on well-separated data, where it does not)."""
    X = tc.fit_series()
    assert len(X) == 240 and min(map(len, X)) >= 20 and max(map(len, X)) <= 60
    ora = O.OracleAnnchor(len(X), lambda IJ: tc.HOSTS[name](X, IJ, **kw), **tc.FIT_CFG).fit()
    assert ora.neighbor_graph[0].shape == (240, 10)
    assert np.all(np.isfinite(ora.neighbor_graph[1]))
