"""Optimal string alignment on the host: the definition's loop against known answers and an integer loop written on its own, the
vectorised helper and the lane-by-lane restatement of the kernel's schedule (csrc/wed.hip, k_osa) against the loop, single swaps
at every position, transpose = +inf against weighted Levenshtein, the triangle inequality's counterexample, the constructor's
refusals and the name lookup.  Every comparison of distances is np.array_equal or ==."""
import numpy as np
import pytest

import osa_cases as oc
import wed_cases as wc


# -------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("x, y, want", [("ab", "ba", 1.0), ("ca", "abc", 3.0), ("abcd", "acbd", 1.0), ("abc", "", 3.0), ("", "", 0.0),
                                        ("aa", "aa", 0.0)])
def test_known_answers(x, y, want):
    """Unit costs.  ("ca", "abc") = 3 is what tells OSA from the unrestricted Damerau-Levenshtein distance, which gives 2."""
    costs = oc.unit(26)
    for a, b in ((x, y), (y, x)):
        assert oc.osa_loop(a, b, costs) == want
        assert oc.osa_pairs_host([a, b], [[0, 1]], costs)[0] == want
        for R, G in oc.SHAPES:
            assert oc.osa_lanes([a, b], [[0, 1]], costs, R, G)[0] == want


def test_loop_equals_an_integer_loop_at_unit_costs():
    """All 364 strings of <= 5 symbols over 3 symbols, all ordered pairs: osa_loop (two rolling rows, row -1 and column -1 as
    sums) against the textbook full-matrix recurrence on integers."""
    X = oc.all_strings(3, 5)
    assert len(X) == 364 and X[0] == ""
    costs = oc.unit(3)
    swaps = 0
    for x in X:
        for y in X:
            d = oc.osa_int_loop(x, y)
            assert oc.osa_loop(x, y, costs) == float(d), (x, y)
            swaps += d < wc.levenshtein_loop(x, y)
    assert swaps > 1000   # the fourth term decides a good share of the pairs


def test_not_a_metric():
    """The counterexample, and metric_violation() naming it; with transpose = +inf the value is weighted Levenshtein's and the
    costs alone decide; a finding on S and g comes first."""
    from annchor_amd.distances import OSA

    u = oc.unit(3)
    ca_abc, ca_ac, ac_abc = (oc.osa_loop(x, y, u) for x, y in (("ca", "abc"), ("ca", "ac"), ("ac", "abc")))
    assert (ca_abc, ca_ac, ac_abc) == (3.0, 1.0, 1.0) and ca_abc > ca_ac + ac_abc
    said = OSA.unit("abc").metric_violation()
    assert said == ('a finite transpose breaks the triangle inequality: at unit costs osa("ca", "abc") = 3 > '
                    'osa("ca", "ac") + osa("ac", "abc") = 2')
    assert oc.metric_of(oc.ragged_costs(5)).metric_violation() == said
    assert OSA("abc", 1.0 - np.eye(3), 1.0, np.inf).metric_violation() is None
    n = wc.nonmetric()
    for T in (1.0, np.inf):
        assert OSA(n.alphabet, n.S, n.g, T).metric_violation() == "substitution[0][1] = 3.0 > substitution[0][2] + substitution[2][1] = 2.0"
    assert OSA("abc", 1.0 - np.eye(3), [1.0, 0.0, 1.0]).metric_violation() == "indel[1] = 0 for the symbol 'b'"


# ---------------------------------------------------------------------- the helper and the kernel's schedule, restated
_LOOP = {}


def loop_ref(X, key, IJ, costs):
    if key not in _LOOP:
        _LOOP[key] = np.array([oc.osa_loop(X[i], X[j], costs) for i, j in IJ])
        _LOOP[key].setflags(write=False)
    return _LOOP[key]


@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_helper_and_lane_model_equal_the_loop(shape, kind):
    """osa_pairs_host and the schedule of k_osa<R, G> on 64 lanes -- both wavefront shifts, the strip, both boundary words and
    their two-step histories, the moved-down x_{i-1} and the two sentinels, the clamps, the slack entry, the flat table --
    against osa_loop, for every (R, G): lengths 0, 1, 2, R-1, R, R+1, 2R, GR-1, GR at the two small shapes and 0, 1, 2, R+1, 1023,
    1024 at the widest, all crossed in both argument orders, under dyadic and under non-dyadic costs, the empty string first and
    last in the pool (the last one's clamped index 0 is the slack entry)."""
    R, G = oc.SHAPES[shape]
    Ls, IJ = oc.lane_case(shape)
    assert max(Ls) == R * G and (shape < 2 or max(Ls) == oc.MAX_LENGTH) and Ls[0] == 0 and Ls[-1] == 0
    costs = oc.dyadic(5, seed=40 + shape) if kind == "dyadic" else oc.ragged_costs(5, seed=40 + shape)
    X = oc.one_of_each_length(Ls, 5, seed=60 + shape)
    want = loop_ref(X, (shape, kind), IJ, costs)
    both = (np.array(Ls)[IJ] > 0).all(axis=1)
    assert np.all(np.isfinite(want)) and np.all(want[both & (IJ[:, 0] != IJ[:, 1])] > 0)
    assert np.array_equal(oc.osa_pairs_host(X, IJ, costs), want)
    assert np.array_equal(oc.osa_lanes(X, IJ, costs, R, G), want)
    # the fourth term is in the values: they differ from weighted Levenshtein's on the same table, never upwards
    wed = wc.wed_pairs_host(X, IJ, oc.wed_part(costs))
    assert np.all(want <= wed) and np.any(want < wed)
    # both argument orders are in the list and agree
    n = len(Ls)
    full = np.full(n * n, np.nan)
    full[IJ[:, 0] * n + IJ[:, 1]] = want
    full = full.reshape(n, n)
    seen = ~np.isnan(full) & ~np.isnan(full.T)
    assert np.array_equal(full[seen], full.T[seen])


@pytest.mark.parametrize("A", [1, 2, 127, 128])
def test_helper_and_lane_model_reach_the_table_ends(A):
    """Code A-1 as row and as column is entry A + A A - 1, the last of the flat image, and g[A-1] the entry before S; at A = 1
    no two adjacent symbols differ and the term, which fires on every cell, changes nothing."""
    costs = oc.below_every_cost(oc.ragged_costs(A, seed=A))
    X = oc.using_every_symbol(A, seed=A)[:12] + oc.using_every_symbol(A, seed=A)[36:]
    X = [""] + X + [X[-1][:3] + X[-1][4] + X[-1][3] + X[-1][5:], ""]      # a swap of the longest string; the empty string first and last
    IJ = oc.all_ordered_pairs(len(X))[::3]
    want = np.array([oc.osa_loop(X[i], X[j], costs) for i, j in IJ])
    assert np.array_equal(oc.osa_pairs_host(X, IJ, costs), want)
    assert np.array_equal(oc.osa_lanes(X, IJ, costs, 8, 16), want)
    assert np.array_equal(oc.osa_lanes(X, IJ[:40], costs, 8, 64), want[:40])
    k = len(X) - 2
    assert A == 1 or X[k] == X[k - 1] or oc.osa_loop(X[k - 1], X[k], costs) == costs.T


# ------------------------------------------------------------------------------------- cases the boundary cannot hide from
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_single_swaps_at_every_position(shape):
    """A base string with no two equal neighbours -- 128 symbols on the (8, 16) shape, 200 on the two others: 25 resp. 13 lanes
    and four strips of y -- and every string obtained from it by swapping positions (p, p+1), p = 0 .. n-2, with T below every
    other cost: osa(base, swapped) == T exactly (0.0 + T + 0.0 + ...; two differing positions need two substitutions or two
    indels otherwise).  The fourth term fires on the cell (p+1, p+1): on every lane's
    row 0 (second boundary word, moved-down x_{i-1}), on every lane's row 1 (top two steps ago), on column 1 (column -1 as the
    source) and on row 1 of lane 0 (row -1 as the source).  Helper and lane model, both argument orders."""
    R, G = oc.SHAPES[shape]
    X, IJ = oc.swap_case(shape)
    n = oc.SWAP_LENGTH[shape]
    assert len(X[0]) == n > 4 * R and len(X) == n + 1 and len(set(X)) == len(X) and len(X[-1]) == R * G and len(IJ) == 2 * (n - 1)
    costs = oc.below_every_cost(oc.ragged_costs(5, seed=80 + shape))
    assert costs.T < costs.g.min() and costs.T < costs.S[~np.eye(5, dtype=bool)].min()
    want = np.full(len(IJ), costs.T)
    assert np.array_equal(oc.osa_pairs_host(X, IJ, costs), want)
    assert np.array_equal(oc.osa_lanes(X, IJ, costs, R, G), want)
    for p in (0, R - 2, R - 1, R, n - 2):     # the loop on the first column, a lane's last rows and first rows, the last cell
        assert oc.osa_loop(X[0], X[1 + p], costs) == costs.T == oc.osa_loop(X[1 + p], X[0], costs)
    # without the fourth term none of them costs T
    assert np.all(wc.wed_pairs_host(X, IJ[:: max(1, len(IJ) // 64)], oc.wed_part(costs)) > costs.T)


# --------------------------------------------------------------------------------------- against weighted Levenshtein
@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
def test_transpose_inf_or_too_large_equals_weighted_levenshtein(kind):
    """min(v, E + inf) = v: transpose = +inf gives wed_loop's bits, and so does a finite T that never wins.  Deleting x_{i-1},
    matching x_i with y_{j-1} and inserting y_j does a swap's job for 2 g[x_{i-1}] <= 2 max(g), so T = 4 max(cost) loses to it
    by 2 max(cost), far beyond any rounding of the sums."""
    A = 5
    w = wc.dyadic(A) if kind == "dyadic" else wc.ragged_costs(A)
    X = oc.one_of_each_length([0, 1, 2, 3, 5, 8, 13, 21, 34, 34, 55, 0], A, seed=11)
    X[5] = X[4][:2] + X[4][3] + X[4][2] + X[4][4]         # a swapped neighbour, so that a cheap T would win
    IJ = oc.all_ordered_pairs(len(X))
    want = np.array([wc.wed_loop(X[i], X[j], w) for i, j in IJ])
    big = 4.0 * float(max(w.g.max(), w.S.max()))
    for T in (np.inf, big):
        costs = oc.with_transpose(w, T)
        assert np.array_equal([oc.osa_loop(X[i], X[j], costs) for i, j in IJ], want)
        assert np.array_equal(oc.osa_pairs_host(X, IJ, costs), want)
        assert np.array_equal(oc.osa_lanes(X, IJ, costs, 8, 16), want)
    assert not np.array_equal(oc.osa_pairs_host(X, IJ, oc.below_every_cost(oc.with_transpose(w, 1.0))), want)


def test_empty_string_is_the_gap_sum():
    costs = oc.ragged_costs(5)
    x = "abcdeedcba"
    e = oc.gap_sums(oc.codes_of(x, costs), costs)[-1]
    assert oc.osa_loop(x, "", costs) == e == oc.osa_loop("", x, costs) == wc.wed_loop(x, "", oc.wed_part(costs))
    assert np.array_equal(oc.osa_pairs_host([x, "", ""], [[0, 1], [1, 0], [1, 2]], costs), [e, e, 0.0])
    for R, G in oc.SHAPES:
        assert np.array_equal(oc.osa_lanes([x, "", ""], [[0, 1], [1, 0], [1, 2]], costs, R, G), [e, e, 0.0])
    assert np.array_equal(oc.osa_lanes(["", ""], [[0, 1], [1, 1]], costs, 8, 16), [0.0, 0.0])


# ----------------------------------------------------------------------------------------------------------- refusals
def _ulp_off():
    S = wc.ragged_costs(4).S.copy()
    S[1, 2] = np.nextafter(S[1, 2], np.inf)
    return S


@pytest.mark.parametrize("alphabet, S, indel, T, match", [
    ("abcd", _ulp_off(), 1.0, 0.5, r"osa: substitution\[1\]\[2\] = .* but substitution\[2\]\[1\] = .*symmetric"),
    ("abc", np.diag([0.0, 0.5, 0.0]), 1.0, 0.5, r"osa: substitution\[1\]\[1\] = 0.5; the diagonal is 0"),
    ("abc", np.array([[0, 1, 1], [1, 0, -1.0], [1, -1.0, 0]]), 1.0, 0.5, r"osa: substitution\[1\]\[2\] = -1.0 is not a finite cost"),
    ("abc", np.array([[0, np.nan, 1], [np.nan, 0, 1], [1, 1, 0]]), 1.0, 0.5, r"osa: substitution\[0\]\[1\] = nan is not a finite cost"),
    ("abc", 1.0 - np.eye(4), 1.0, 0.5, r"osa: substitution has shape \(4, 4\); the alphabet of 3 symbols needs \(3, 3\)"),
    (wc.SYMBOLS + "!", 1.0 - np.eye(129), 1.0, 0.5, r"osa: the alphabet has 129 symbols; 1 \.\. 128"),
    ("", np.zeros((0, 0)), 1.0, 0.5, r"osa: the alphabet has 0 symbols"),
    ("abca", 1.0 - np.eye(4), 1.0, 0.5, r"osa: alphabet entries 0 and 3 are both 'a'"),
    (["a", "bc"], 1.0 - np.eye(2), 1.0, 0.5, r"osa: alphabet entry 1 is 'bc', not a one-character string"),
    ("abc", 1.0 - np.eye(3), [1.0, 1.0], 0.5, r"osa: indel has shape \(2,\); a scalar or \(3,\)"),
    ("abc", 1.0 - np.eye(3), [1.0, -0.5, 1.0], 0.5, r"osa: indel\[1\] = -0.5 is not a finite cost"),
    ("abc", 1.0 - np.eye(3), np.inf, 0.5, r"osa: indel\[0\] = inf is not a finite cost"),
    ("abc", 1.0 - np.eye(3), "x", 0.5, r"osa: substitution and indel must be arrays of real numbers"),
    ("abc", 1.0 - np.eye(3), 1.0, -0.5, r"osa: transpose = -0.5 is not a cost >= 0 \(inf: no transpositions\)"),
    ("abc", 1.0 - np.eye(3), 1.0, np.nan, r"osa: transpose = nan is not a cost >= 0"),
    ("abc", 1.0 - np.eye(3), 1.0, -np.inf, r"osa: transpose = -inf is not a cost >= 0"),
    ("abc", 1.0 - np.eye(3), 1.0, [0.5, 0.5, 0.5], r"osa: transpose has shape \(3,\); a scalar"),
    ("abc", 1.0 - np.eye(3), 1.0, "x", r"osa: transpose must be a real number"),
])
def test_constructor_refuses(alphabet, S, indel, T, match):
    from annchor_amd.distances import OSA

    with pytest.raises(ValueError, match=match):
        OSA(alphabet, S, indel, T)


def test_constructor_takes():
    from annchor_amd.distances import OSA, DeviceMetric

    w = OSA(["x", "y"], [[0, 2], [2, 0]], indel=3, transpose=2)
    assert isinstance(w, DeviceMetric) and w.name == "osa" and w.ragged
    assert w.substitution.dtype == np.float64 and np.array_equal(w.indel, [3.0, 3.0]) and w.symbols == ["x", "y"]
    assert isinstance(w.transpose, float) and w.transpose == 2.0
    d = OSA("xy", [[0, 2], [2, 0]])
    assert np.array_equal(d.indel, [1.0, 1.0]) and d.transpose == 1.0
    assert OSA("xy", [[0, 2], [2, 0]], transpose=np.inf).transpose == np.inf      # "no transpositions"
    z = OSA("ab", [[-0.0, 1], [1, 0.0]], transpose=-0.0)            # (a negative zero is a zero)
    assert not np.signbit(z.substitution).any() and not np.signbit(z.transpose) and z.transpose == 0.0
    u = OSA.unit(wc.SYMBOLS)
    assert u.indel.shape == (128,) and np.array_equal(u.substitution, 1.0 - np.eye(128)) and u.transpose == 1.0


@pytest.mark.parametrize("X, alphabet, match", [
    (["abc", "abd", "abc"], "abc", r"osa: string 1 holds the symbol 'd', which is not in the alphabet"),
    (["a", "b" * 1025], "ab", r"osa: string 1 has 1025 symbols; at most 1024"),
    (["a", b"ab"], "ab", r"osa: string 1 is a bytes, not a str"),
    (["a", None], "ab", r"osa: string 1 is a NoneType, not a str"),
    ([], "ab", r"osa: no strings"),
])
def test_bind_refuses_on_the_host(X, alphabet, match):
    """OSA.bind packs before it touches the engine: the refusals need none."""
    from annchor_amd.distances import OSA

    A = len(alphabet)
    with pytest.raises(ValueError, match=match):
        OSA(alphabet, 1.0 - np.eye(A)).bind(None, X)


def test_the_limit_itself_is_packed():
    from annchor_amd.distances import OSA_MAX_LENGTH, pack_coded_strings

    assert OSA_MAX_LENGTH == oc.MAX_LENGTH == 1024
    long = oc.one_of_each_length([1024], 128, seed=1)
    codes, _, lens = pack_coded_strings(long + ["a"], wc.SYMBOLS, "osa", OSA_MAX_LENGTH)
    assert list(lens) == [1024, 1] and np.array_equal(codes[:1024], [wc.SYMBOLS.index(ch) for ch in long[0]])


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    costs = oc.dyadic(4)
    f = get_function_from_input("osa", oc.kwargs_of(costs))
    assert isinstance(f, distances.OSA) and isinstance(f, distances.DeviceMetric)
    assert f.name == "osa" and f.ragged
    assert np.array_equal(f.substitution, costs.S) and np.array_equal(f.indel, costs.g) and f.transpose == costs.T
    assert "".join(f.symbols) == costs.alphabet
    h = get_function_from_input("osa", {"alphabet": "ab", "substitution": [[0, 2], [2, 0]]})
    assert np.array_equal(h.indel, [1.0, 1.0]) and h.transpose == 1.0
    assert not hasattr(distances, "osa")          # no default costs, no module-level instance
    for kw in (None, {}, {"alphabet": "ab"}, {"substitution": [[0, 1], [1, 0]]}):
        with pytest.raises(AssertionError, match="osa metric requires alphabet and substitution kwargs"):
            get_function_from_input("osa", kw)
    with pytest.raises(ValueError, match="osa: transpose = -1.0"):
        get_function_from_input("osa", {"alphabet": "ab", "substitution": [[0, 1], [1, 0]], "transpose": -1.0})
    with pytest.raises(AssertionError, match="The string must be one of .*'osa'"):
        get_function_from_input("damerau", None)


def test_fit_data_is_usable():
    """The fit data set of the GPU tests: 240 strings of 20 .. 60 symbols over 12 symbols, T below every other cost; finite
    distances, a zero diagonal, distinct off-diagonal distances within every row (the index comparisons rest on no tie rule),
    and a good share of the pairs -- of the near ones above all, which a fit evaluates -- decided by the fourth term."""
    X, costs = oc.fit_strings(), oc.fit_costs()
    nx = len(X)
    assert nx == 240 and min(map(len, X)) >= 20 and max(map(len, X)) <= 60 and len(costs.alphabet) == 12
    assert costs.T == oc.FIT_T < min(costs.g.min(), costs.S[~np.eye(12, dtype=bool)].min())
    iu = np.triu_indices(nx)
    T = np.zeros((nx, nx))
    T[iu] = oc.osa_pairs_host(X, np.stack(iu, axis=1), costs)
    T.T[iu] = T[iu]
    assert np.all(np.isfinite(T)) and np.all(np.diag(T) == 0.0)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)
    W = np.zeros((nx, nx))
    W[iu] = wc.wed_pairs_host(X, np.stack(iu, axis=1), oc.wed_part(costs))
    W.T[iu] = W[iu]
    assert np.all(T <= W) and (T < W).mean() > 0.3
    near = np.argsort(T, axis=1)[:, 1:11]
    rows = np.arange(nx)[:, None]
    assert (T[rows, near] < W[rows, near]).mean() > 0.5
