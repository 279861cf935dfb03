"""Affine-gap alignment distance on the host: the definition's loop against the enumeration of alignments, the vectorised helper
and the lane-by-lane restatement of the kernel's schedule (csrc/wed.hip, k_affine) against the loop, open = 0 against weighted
Levenshtein, the triangle inequality on small string sets, the empty string, the constructor's refusals and the name lookup.
Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import affine_cases as ac
import wed_cases as wc


# -------------------------------------------------------------------------------------------------- the references
def test_loop_equals_the_enumeration_of_alignments():
    """All 31 strings of <= 4 symbols over 2 symbols, all ordered pairs, dyadic costs (every sum is exact, so the path's order of
    additions and the recurrence's give the same bits), at open = 0.75 and at open = 0."""
    X = ac.all_strings(2, 4)
    assert len(X) == 31 and X[0] == ""
    for o in (ac.DYADIC_OPEN, 0.0):
        costs = ac.dyadic(2, o=o)
        for x in X:
            for y in X:
                assert ac.affine_loop(x, y, costs) == ac.affine_by_enumeration(x, y, costs), (x, y, o)


@pytest.mark.parametrize("x, y, o, want", [("", "", 2.0, 0.0), ("abc", "", 2.0, 5.0), ("abc", "abc", 2.0, 0.0), ("a", "abbb", 2.0, 5.0),
                                           ("abbba", "aa", 0.5, 3.5), ("ab", "ba", 3.0, 2.0), ("ab", "ba", 0.25, 2.0)])
def test_known_answers(x, y, o, want):
    """Unit substitutions and extensions: one gap of k symbols costs o + k, and two substitutions beat two gaps."""
    costs = ac.with_open(wc.unit(26), o)
    for a, b in ((x, y), (y, x)):
        assert ac.affine_loop(a, b, costs) == want
        assert ac.affine_pairs_host([a, b], [[0, 1]], costs)[0] == want


@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
def test_helper_equals_the_loop(kind):
    """All length pairs in 0..12 and a few up to 70 -- the empty string among them, twice -- in both argument orders (all ordered
    pairs), bit for bit; the matrix is symmetric bit for bit and its diagonal 0."""
    A = 5
    costs = ac.dyadic(A) if kind == "dyadic" else ac.ragged_costs(A)
    X = ac.one_of_each_length([0] + list(range(0, 13)) + [31, 47, 70], A, seed=3)
    IJ = ac.all_ordered_pairs(len(X))
    got = ac.affine_pairs_host(X, IJ, costs)
    want = np.array([ac.affine_loop(X[i], X[j], costs) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    assert got[0 * len(X) + 1] == 0.0                      # affine("", "") between two members
    assert np.all(got[(IJ[:, 0] != IJ[:, 1]) & (IJ.min(axis=1) > 1)] > 0.0)
    # the opening cost is in the values: they differ from weighted Levenshtein's on the same table
    assert not np.array_equal(got, wc.wed_pairs_host(X, IJ, ac.wed_part(costs)))


def test_empty_string_is_the_sum_from_open():
    """affine(x, "") = ((o + g[x_0]) + g[x_1]) + ..., left to right."""
    costs = ac.ragged_costs(5)
    x = "abcdeedcba"
    e = costs.o
    for a in ac.codes_of(x, costs):
        e = e + costs.g[a]
    assert e == ac.gap_sums(ac.codes_of(x, costs), costs)[-1] and e > wc.wed_loop(x, "", ac.wed_part(costs))
    assert ac.affine_loop(x, "", costs) == e == ac.affine_loop("", x, costs)
    assert np.array_equal(ac.affine_pairs_host([x, "", ""], [[0, 1], [1, 0], [1, 2]], costs), [e, e, 0.0])
    for R, G in ac.SHAPES:
        assert np.array_equal(ac.affine_lanes([x, "", ""], [[0, 1], [1, 0], [1, 2]], costs, R, G), [e, e, 0.0])


@pytest.mark.parametrize("kind", ["dyadic", "ragged"])
def test_open_zero_equals_weighted_levenshtein(kind):
    """H + 0.0 == H and P(i-1, j) >= H(i-1, j): with open = 0.0 the three states collapse into wed's one, bit for bit."""
    A = 5
    w = wc.dyadic(A) if kind == "dyadic" else wc.ragged_costs(A)
    costs = ac.with_open(w, 0.0)
    X = ac.one_of_each_length([0, 1, 2, 3, 5, 8, 13, 21, 34, 34, 55], A, seed=11)
    IJ = ac.all_ordered_pairs(len(X))
    want = np.array([wc.wed_loop(X[i], X[j], w) for i, j in IJ])
    assert np.array_equal([ac.affine_loop(X[i], X[j], costs) for i, j in IJ], want)
    assert np.array_equal(ac.affine_pairs_host(X, IJ, costs), want)
    assert np.array_equal(ac.affine_lanes(X, IJ, costs, 8, 16), want)


# ---------------------------------------------------------------------------------------- the kernel's schedule, restated
_LOOP = {}


def loop_ref(X, key, i, j, costs):
    k = (key, i, j)
    if k not in _LOOP:
        _LOOP[k] = ac.affine_loop(X[i], X[j], costs)
    return _LOOP[k]


def lane_case(shape):
    """(lengths, pair list) of one shape: every length crossed with every length, minus the last pair at the narrow shape with 4
    pairs per wavefront, so that its last wavefront has inactive slots."""
    R, G = ac.SHAPES[shape]
    Ls = [0, 1, R - 1, R, R + 1, 2 * R, G * R - 1, G * R] if shape < 2 else [0, 1, R + 1, ac.MAX_LENGTH - 1, ac.MAX_LENGTH]
    IJ = ac.all_ordered_pairs(len(Ls))
    if G < ac.WAVE:
        IJ = IJ[:-1]
        assert len(IJ) % (ac.WAVE // G) != 0
    return Ls, IJ


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_lane_by_lane_restatement_equals_the_loop(shape):
    """The schedule of k_affine<R, G> on 64 lanes -- both wavefront shifts, the strip, the two-word boundary between lanes, the q
    rows, H(-1, .) with P = +inf arriving at lane 0, the sums from o at column -1 -- against affine_loop, for every (R, G):
    lengths 0, 1, R-1, R, R+1, 2R, GR-1, GR at the two small shapes and 0, 1, R+1, 1023, 1024 at the widest, all crossed in both
    orders, non-dyadic costs and open, the empty string first in the pool."""
    R, G = ac.SHAPES[shape]
    Ls, IJ = lane_case(shape)
    assert max(Ls) == R * G and (shape < 2 or max(Ls) == ac.MAX_LENGTH)
    costs = ac.ragged_costs(5, seed=40 + shape)
    X = ac.one_of_each_length(Ls, 5, seed=60 + shape)
    got = ac.affine_lanes(X, IJ, costs, R, G)
    want = np.array([loop_ref(X, shape, i, j, costs) for i, j in IJ])
    assert np.all(np.isfinite(want)) and np.all(want[IJ[:, 0] != IJ[:, 1]] > 0)
    assert np.array_equal(got, want)


def test_lane_by_lane_restatement_with_an_empty_last_member():
    """The empty string LAST in the pool: its clamped index 0 is the slack entry behind the pool.  And a list of empty strings
    only."""
    costs = ac.ragged_costs(3, seed=7)
    X = ac.one_of_each_length([9, 1, 20, 0], 3, seed=8)
    IJ = ac.all_ordered_pairs(4)
    want = np.array([ac.affine_loop(X[i], X[j], costs) for i, j in IJ])
    for R, G in ac.SHAPES:
        assert np.array_equal(ac.affine_lanes(X, IJ, costs, R, G), want)
    assert np.array_equal(ac.affine_lanes(["", ""], [[0, 1], [1, 1]], costs, 8, 16), [0.0, 0.0])


@pytest.mark.parametrize("A", [1, 2, 127, 128])
def test_lane_by_lane_restatement_reaches_the_table_ends(A):
    """Code A-1 as row and as column is entry A + A A - 1, the last of the flat image, and g[A-1] the entry before S."""
    costs = ac.ragged_costs(A, seed=A)
    X = ac.using_every_symbol(A, seed=A)[:12] + ac.using_every_symbol(A, seed=A)[36:]
    IJ = ac.all_ordered_pairs(len(X))[::3]
    want = np.array([ac.affine_loop(X[i], X[j], costs) for i, j in IJ])
    assert np.array_equal(ac.affine_lanes(X, IJ, costs, 8, 16), want)


# --------------------------------------------------------------------------------------------------------- a metric
@pytest.mark.parametrize("A, longest, count", [(2, 5, 63), (3, 4, 121)])
@pytest.mark.parametrize("o", [0.0, 0.25, 0.75, 3.0])
def test_triangle_inequality_on_every_small_string(A, longest, count, o):
    """Every string of <= 5 symbols over 2 symbols (63) and of <= 4 over 3 (121), every triple, dyadic costs under which
    metric_violation() is None -- the sums are exact, so the inequality is tested with no slack: d(a, c) <= d(a, b) + d(b, c);
    and d is symmetric, 0 on the diagonal and positive off it."""
    costs = ac.dyadic(A, o=o)
    assert ac.metric_of(costs).metric_violation() is None
    X = ac.all_strings(A, longest)
    assert len(X) == count
    T = ac.affine_pairs_host(X, ac.all_ordered_pairs(count), costs).reshape(count, count)
    assert np.array_equal(T, T.T) and np.all(np.diag(T) == 0.0) and np.all(T[~np.eye(count, dtype=bool)] > 0.0)
    for b in range(count):
        assert np.all(T <= T[:, b, None] + T[None, b, :]), X[b]


def test_metric_violation():
    from annchor_amd.distances import AffineGap

    for A in (1, 2, 5, 26, 128):
        assert ac.metric_of(ac.dyadic(A)).metric_violation() is None
        assert ac.metric_of(ac.ragged_costs(A)).metric_violation() is None
    n = wc.nonmetric()
    assert (AffineGap(n.alphabet, n.S, n.g, 1.0).metric_violation()
            == "substitution[0][1] = 3.0 > substitution[0][2] + substitution[2][1] = 2.0")
    S = 1.0 - np.eye(3)
    assert AffineGap("abc", S, [1.0, 0.0, 1.0], 0.5).metric_violation() == "extend[1] = 0 for the symbol 'b'"
    assert AffineGap("abc", S, [1.0, 3.0, 1.0]).metric_violation() == "extend[1] = 3.0 > substitution[1][0] + extend[0] = 2.0"
    S[1, 2] = S[2, 1] = 1.5
    assert AffineGap("abc", S, [1.0, 0.25, 1.0]).metric_violation() == "substitution[1][2] = 1.5 > extend[1] + extend[2] = 1.25"


# ----------------------------------------------------------------------------------------------------------- refusals
def _ulp_off():
    S = wc.ragged_costs(4).S.copy()
    S[1, 2] = np.nextafter(S[1, 2], np.inf)
    return S


@pytest.mark.parametrize("alphabet, S, extend, o, match", [
    ("abcd", _ulp_off(), 1.0, 0.5, r"affine_gap: substitution\[1\]\[2\] = .* but substitution\[2\]\[1\] = .*symmetric"),
    ("abc", np.diag([0.0, 0.5, 0.0]), 1.0, 0.5, r"affine_gap: substitution\[1\]\[1\] = 0.5; the diagonal is 0"),
    ("abc", np.array([[0, 1, 1], [1, 0, -1.0], [1, -1.0, 0]]), 1.0, 0.5, r"affine_gap: substitution\[1\]\[2\] = -1.0 is not a finite cost"),
    ("abc", np.array([[0, np.nan, 1], [np.nan, 0, 1], [1, 1, 0]]), 1.0, 0.5, r"affine_gap: substitution\[0\]\[1\] = nan is not a finite cost"),
    ("abc", 1.0 - np.eye(4), 1.0, 0.5, r"affine_gap: substitution has shape \(4, 4\); the alphabet of 3 symbols needs \(3, 3\)"),
    (wc.SYMBOLS + "!", 1.0 - np.eye(129), 1.0, 0.5, r"affine_gap: the alphabet has 129 symbols; 1 \.\. 128"),
    ("", np.zeros((0, 0)), 1.0, 0.5, r"affine_gap: the alphabet has 0 symbols"),
    ("abca", 1.0 - np.eye(4), 1.0, 0.5, r"affine_gap: alphabet entries 0 and 3 are both 'a'"),
    (["a", "bc"], 1.0 - np.eye(2), 1.0, 0.5, r"affine_gap: alphabet entry 1 is 'bc', not a one-character string"),
    ("abc", 1.0 - np.eye(3), [1.0, 1.0], 0.5, r"affine_gap: extend has shape \(2,\); a scalar or \(3,\)"),
    ("abc", 1.0 - np.eye(3), [1.0, -0.5, 1.0], 0.5, r"affine_gap: extend\[1\] = -0.5 is not a finite cost"),
    ("abc", 1.0 - np.eye(3), np.inf, 0.5, r"affine_gap: extend\[0\] = inf is not a finite cost"),
    ("abc", 1.0 - np.eye(3), "x", 0.5, r"affine_gap: substitution and extend must be arrays of real numbers"),
    ("abc", 1.0 - np.eye(3), 1.0, -0.5, r"affine_gap: open = -0.5 is not a finite cost >= 0"),
    ("abc", 1.0 - np.eye(3), 1.0, np.nan, r"affine_gap: open = nan is not a finite cost >= 0"),
    ("abc", 1.0 - np.eye(3), 1.0, np.inf, r"affine_gap: open = inf is not a finite cost >= 0"),
    ("abc", 1.0 - np.eye(3), 1.0, [0.5, 0.5, 0.5], r"affine_gap: open has shape \(3,\); a scalar"),
    ("abc", 1.0 - np.eye(3), 1.0, "x", r"affine_gap: open must be a real number"),
])
def test_constructor_refuses(alphabet, S, extend, o, match):
    from annchor_amd.distances import AffineGap

    with pytest.raises(ValueError, match=match):
        AffineGap(alphabet, S, extend, o)


def test_constructor_takes():
    from annchor_amd.distances import AffineGap, DeviceMetric

    w = AffineGap(["x", "y"], [[0, 2], [2, 0]], extend=3, open=2)
    assert isinstance(w, DeviceMetric) and w.name == "affine_gap" and w.ragged
    assert w.substitution.dtype == np.float64 and np.array_equal(w.extend, [3.0, 3.0]) and w.symbols == ["x", "y"]
    assert isinstance(w.open, float) and w.open == 2.0
    d = AffineGap("xy", [[0, 2], [2, 0]])
    assert np.array_equal(d.extend, [1.0, 1.0]) and d.open == 0.0
    z = AffineGap("ab", [[-0.0, 1], [1, 0.0]], open=-0.0)          # (a negative zero is a zero)
    assert not np.signbit(z.substitution).any() and not np.signbit(z.open)
    assert AffineGap(wc.SYMBOLS, 1.0 - np.eye(128)).extend.shape == (128,)


@pytest.mark.parametrize("X, alphabet, match", [
    (["abc", "abd", "abc"], "abc", r"affine_gap: string 1 holds the symbol 'd', which is not in the alphabet"),
    (["a", "b" * 1025], "ab", r"affine_gap: string 1 has 1025 symbols; at most 1024"),
    (["a", b"ab"], "ab", r"affine_gap: string 1 is a bytes, not a str"),
    (["a", None], "ab", r"affine_gap: string 1 is a NoneType, not a str"),
    ([], "ab", r"affine_gap: no strings"),
])
def test_bind_refuses_on_the_host(X, alphabet, match):
    """AffineGap.bind packs before it touches the engine: the refusals need none."""
    from annchor_amd.distances import AffineGap

    A = len(alphabet)
    with pytest.raises(ValueError, match=match):
        AffineGap(alphabet, 1.0 - np.eye(A)).bind(None, X)


def test_the_limit_itself_is_packed():
    from annchor_amd.distances import AFFINE_MAX_LENGTH, pack_coded_strings

    assert AFFINE_MAX_LENGTH == ac.MAX_LENGTH == 1024
    long = ac.one_of_each_length([1024], 128, seed=1)
    codes, _, lens = pack_coded_strings(long + ["a"], wc.SYMBOLS, "affine_gap", AFFINE_MAX_LENGTH)
    assert list(lens) == [1024, 1] and np.array_equal(codes[:1024], [wc.SYMBOLS.index(ch) for ch in long[0]])


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    costs = ac.dyadic(4)
    f = get_function_from_input("affine_gap", ac.kwargs_of(costs))
    assert isinstance(f, distances.AffineGap) and isinstance(f, distances.DeviceMetric)
    assert f.name == "affine_gap" and f.ragged
    assert np.array_equal(f.substitution, costs.S) and np.array_equal(f.extend, costs.g) and f.open == costs.o
    assert "".join(f.symbols) == costs.alphabet
    h = get_function_from_input("affine_gap", {"alphabet": "ab", "substitution": [[0, 2], [2, 0]]})
    assert np.array_equal(h.extend, [1.0, 1.0]) and h.open == 0.0
    assert not hasattr(distances, "affine_gap")          # no default costs, no module-level instance
    for kw in (None, {}, {"alphabet": "ab"}, {"substitution": [[0, 1], [1, 0]]}):
        with pytest.raises(AssertionError, match="affine_gap metric requires alphabet and substitution kwargs"):
            get_function_from_input("affine_gap", kw)
    with pytest.raises(ValueError, match="affine_gap: open = -1.0"):
        get_function_from_input("affine_gap", {"alphabet": "ab", "substitution": [[0, 1], [1, 0]], "open": -1.0})


def test_fit_data_is_usable():
    """The fit data set of the GPU tests under the affine costs: finite distances, a zero diagonal, distinct off-diagonal
    distances within every row (the index comparisons rest on no tie rule), the triangle inequality on sampled triples."""
    X, costs = ac.fit_strings(), ac.fit_costs()
    nx = len(X)
    assert nx == 240 and costs.o == 0.7 and ac.metric_of(costs).metric_violation() is None
    iu = np.triu_indices(nx)
    T = np.zeros((nx, nx))
    T[iu] = ac.affine_pairs_host(X, np.stack(iu, axis=1), costs)
    T.T[iu] = T[iu]
    assert np.all(np.isfinite(T)) and np.all(np.diag(T) == 0.0)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)
    rng = np.random.default_rng(7)
    a, b, c = rng.integers(0, nx, size=(3, 5000))
    assert np.all(T[a, c] <= (T[a, b] + T[b, c]) * (1 + 1e-12))
