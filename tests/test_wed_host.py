"""Weighted Levenshtein on the host: the vectorised helper and the lane-by-lane restatement of the kernel's schedule
(csrc/wed.hip) against the plain double loop of wed_cases.py, unit costs against a plain Levenshtein loop, metric_violation(),
the constructor's and the packer's refusals, and the name lookup.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import wed_cases as wc


def cost_sets(A):
    return {"unit": wc.unit(A), "dyadic": wc.dyadic(A), "ragged": wc.ragged_costs(A)}


# ------------------------------------------------------------------------------------------------- the two references
@pytest.mark.parametrize("kind", ["unit", "dyadic", "ragged"])
def test_helper_equals_the_double_loop(kind):
    """All length pairs in 0..12 and a few up to 70 -- the empty string among them, twice -- in both argument orders (all ordered
    pairs), bit for bit; the matrix is symmetric bit for bit and its diagonal 0."""
    A = 5
    costs = cost_sets(A)[kind]
    X = wc.one_of_each_length([0] + list(range(0, 13)) + [31, 47, 70], A, seed=3)
    IJ = wc.all_ordered_pairs(len(X))
    got = wc.wed_pairs_host(X, IJ, costs)
    want = np.array([wc.wed_loop(X[i], X[j], costs) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    assert got[0 * len(X) + 1] == 0.0                      # wed("", "") between two members
    assert np.all(got[(IJ[:, 0] != IJ[:, 1]) & (IJ.min(axis=1) > 1)] > 0.0)


@pytest.mark.parametrize("x, y, want", [("", "", 0.0), ("abc", "", 3.0), ("abc", "abc", 0.0), ("kitten", "sitting", 3.0), ("a", "bb", 2.0)])
def test_known_answers(x, y, want):
    costs = wc.unit(26)
    for a, b in ((x, y), (y, x)):
        assert wc.wed_loop(a, b, costs) == want
        assert wc.wed_pairs_host([a, b], [[0, 1]], costs)[0] == want


def test_empty_string_is_the_gap_sum():
    costs = wc.ragged_costs(5)
    x = "abcdeedcba"
    gs = wc.gap_sums(wc.codes_of(x, costs), costs)
    assert wc.wed_loop(x, "", costs) == gs[-1] == wc.wed_loop("", x, costs)
    assert np.array_equal(wc.wed_pairs_host([x, "", ""], [[0, 1], [1, 0], [1, 2]], costs), [gs[-1], gs[-1], 0.0])


def test_unit_costs_equal_plain_levenshtein():
    A = 4
    X = wc.one_of_each_length([0, 1, 2, 5, 9, 17, 30, 30, 41], A, seed=5)
    IJ = wc.all_ordered_pairs(len(X))
    want = np.array([wc.levenshtein_loop(X[i], X[j]) for i, j in IJ], dtype=np.float64)
    assert np.array_equal(wc.wed_pairs_host(X, IJ, wc.unit(A)), want)
    assert np.array_equal([wc.wed_loop(X[i], X[j], wc.unit(A)) for i, j in IJ], want)


# ---------------------------------------------------------------------------------------- the kernel's schedule, restated
_LOOP = {}


def loop_ref(X, key, i, j, costs):
    k = (key, i, j)
    if k not in _LOOP:
        _LOOP[k] = wc.wed_loop(X[i], X[j], costs)
    return _LOOP[k]


def lane_case(shape):
    """(lengths, pair list) of one shape: every length crossed with every length, minus the last pair at the narrow shape with 4
    pairs per wavefront, so that its last wavefront has inactive slots."""
    R, G = wc.SHAPES[shape]
    Ls = [0, 1, R - 1, R, R + 1, 2 * R, G * R - 1, G * R] if shape < 2 else [0, 1, R + 1, wc.MAX_LENGTH - 1, wc.MAX_LENGTH]
    IJ = wc.all_ordered_pairs(len(Ls))
    if G < wc.WAVE:
        IJ = IJ[:-1]
        assert len(IJ) % (wc.WAVE // G) != 0
    return Ls, IJ


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_lane_by_lane_restatement_equals_the_double_loop(shape):
    """The schedule of k_wed<R, G> on 64 lanes -- both wavefront shifts, the strip, E(-1, .) arriving at lane 0, E(., -1) at column
    -1, the flat table index -- against wed_loop, for every (R, G): lengths 0, 1, R-1, R, R+1, 2R, GR-1, GR at the two small
    shapes and 0, 1, R+1, 2047, 2048 at the widest, all crossed in both orders, non-dyadic costs, the empty string first in the
    pool (its partner's slot shares a wavefront with running pairs at the 4-pairs shape)."""
    R, G = wc.SHAPES[shape]
    Ls, IJ = lane_case(shape)
    costs = wc.ragged_costs(5, seed=40 + shape)
    X = wc.one_of_each_length(Ls, 5, seed=60 + shape)
    got = wc.wed_lanes(X, IJ, costs, R, G)
    want = np.array([loop_ref(X, shape, i, j, costs) for i, j in IJ])
    assert np.all(np.isfinite(want)) and np.all(want[IJ[:, 0] != IJ[:, 1]] > 0)
    assert np.array_equal(got, want)


def test_lane_by_lane_restatement_with_an_empty_last_member():
    """The empty string LAST in the pool: its clamped index 0 is the slack entry behind the pool.  And a list of empty strings
    only."""
    costs = wc.ragged_costs(3, seed=7)
    X = wc.one_of_each_length([9, 1, 20, 0], 3, seed=8)
    IJ = wc.all_ordered_pairs(4)
    want = np.array([wc.wed_loop(X[i], X[j], costs) for i, j in IJ])
    for R, G in wc.SHAPES[:2]:
        assert np.array_equal(wc.wed_lanes(X, IJ, costs, R, G), want)
    assert np.array_equal(wc.wed_lanes(["", ""], [[0, 1], [1, 1]], costs, 8, 16), [0.0, 0.0])


@pytest.mark.parametrize("A", [1, 2, 127, 128])
def test_lane_by_lane_restatement_reaches_the_table_ends(A):
    """Code A-1 as row and as column is entry A + A A - 1, the last of the flat image, and g[A-1] the entry before S."""
    costs = wc.ragged_costs(A, seed=A)
    X = wc.using_every_symbol(A, seed=A)[:12] + wc.using_every_symbol(A, seed=A)[36:]
    IJ = wc.all_ordered_pairs(len(X))[::3]
    want = np.array([wc.wed_loop(X[i], X[j], costs) for i, j in IJ])
    assert np.array_equal(wc.wed_lanes(X, IJ, costs, 8, 16), want)


# --------------------------------------------------------------------------------------------------- metric_violation
@pytest.mark.parametrize("A", [1, 2, 5, 26, 128])
def test_metric_violation_is_none_for_the_metric_cost_sets(A):
    for kind, costs in cost_sets(A).items():
        assert wc.metric_of(costs).metric_violation() is None, kind
    r = wc.ragged_costs(A)
    if A > 1:
        off = r.S[~np.eye(A, dtype=bool)]
        assert np.all(off > 0) and not np.all(off * 4 == np.round(off * 4))   # (positive, and not dyadic)


def test_metric_violation_names_the_violation():
    from annchor_amd.distances import WeightedLevenshtein

    v = wc.metric_of(wc.nonmetric()).metric_violation()
    assert v == "substitution[0][1] = 3.0 > substitution[0][2] + substitution[2][1] = 2.0"
    S = 1.0 - np.eye(3)
    S[0, 2] = S[2, 0] = 0.0
    assert WeightedLevenshtein("abc", S, 1.0).metric_violation() == "substitution[0][2] = 0 between the distinct symbols 'a' and 'c'"
    S = 1.0 - np.eye(3)
    S[1, 2] = S[2, 1] = 1.5
    assert WeightedLevenshtein("abc", S, [1.0, 0.25, 1.0]).metric_violation() == "substitution[1][2] = 1.5 > indel[1] + indel[2] = 1.25"
    assert WeightedLevenshtein("abc", 1.0 - np.eye(3), [1.0, 0.0, 1.0]).metric_violation() == "indel[1] = 0 for the symbol 'b'"
    assert (WeightedLevenshtein("abc", 1.0 - np.eye(3), [1.0, 3.0, 1.0]).metric_violation()
            == "indel[1] = 3.0 > substitution[1][0] + indel[0] = 2.0")


def test_a_broken_triangle_shows_in_the_values():
    """The nonmetric costs give distances that break the triangle inequality: a -> b costs 3 directly and is what the recurrence
    charges, while a -> c -> b costs 2."""
    costs = wc.nonmetric()
    a, b, c = costs.alphabet[:3]
    assert wc.wed_loop(a, b, costs) == 3.0 and wc.wed_loop(a, c, costs) + wc.wed_loop(c, b, costs) == 2.0


# ----------------------------------------------------------------------------------------------------------- refusals
def _ulp_off():
    S = wc.ragged_costs(4).S.copy()
    S[1, 2] = np.nextafter(S[1, 2], np.inf)
    return S


@pytest.mark.parametrize("alphabet, S, indel, match", [
    ("abcd", _ulp_off(), 1.0, r"weighted_levenshtein: substitution\[1\]\[2\] = .* but substitution\[2\]\[1\] = .*symmetric"),
    ("abc", np.diag([0.0, 0.5, 0.0]), 1.0, r"weighted_levenshtein: substitution\[1\]\[1\] = 0.5; the diagonal is 0"),
    ("abc", np.array([[0, 1, 1], [1, 0, -1.0], [1, -1.0, 0]]), 1.0, r"weighted_levenshtein: substitution\[1\]\[2\] = -1.0 is not a finite cost"),
    ("abc", np.array([[0, np.nan, 1], [np.nan, 0, 1], [1, 1, 0]]), 1.0, r"weighted_levenshtein: substitution\[0\]\[1\] = nan is not a finite cost"),
    ("abc", np.array([[0, np.inf, 1], [np.inf, 0, 1], [1, 1, 0]]), 1.0, r"weighted_levenshtein: substitution\[0\]\[1\] = inf is not a finite cost"),
    ("abc", 1.0 - np.eye(4), 1.0, r"weighted_levenshtein: substitution has shape \(4, 4\); the alphabet of 3 symbols needs \(3, 3\)"),
    ("abc", np.zeros(9), 1.0, r"weighted_levenshtein: substitution has shape \(9,\)"),
    (wc.SYMBOLS + "!", 1.0 - np.eye(129), 1.0, r"weighted_levenshtein: the alphabet has 129 symbols; 1 \.\. 128"),
    ("", np.zeros((0, 0)), 1.0, r"weighted_levenshtein: the alphabet has 0 symbols"),
    ("abca", 1.0 - np.eye(4), 1.0, r"weighted_levenshtein: alphabet entries 0 and 3 are both 'a'"),
    (["a", "bc"], 1.0 - np.eye(2), 1.0, r"weighted_levenshtein: alphabet entry 1 is 'bc', not a one-character string"),
    (["a", 7], 1.0 - np.eye(2), 1.0, r"weighted_levenshtein: alphabet entry 1 is 7, not a one-character string"),
    ("abc", 1.0 - np.eye(3), [1.0, 1.0], r"weighted_levenshtein: indel has shape \(2,\); a scalar or \(3,\)"),
    ("abc", 1.0 - np.eye(3), [1.0, -0.5, 1.0], r"weighted_levenshtein: indel\[1\] = -0.5 is not a finite cost"),
    ("abc", 1.0 - np.eye(3), np.nan, r"weighted_levenshtein: indel\[0\] = nan is not a finite cost"),
])
def test_constructor_refuses(alphabet, S, indel, match):
    from annchor_amd.distances import WeightedLevenshtein

    with pytest.raises(ValueError, match=match):
        WeightedLevenshtein(alphabet, S, indel)


def test_constructor_takes():
    from annchor_amd.distances import DeviceMetric, WeightedLevenshtein

    w = WeightedLevenshtein(["x", "y"], [[0, 2], [2, 0]], indel=3)
    assert isinstance(w, DeviceMetric) and w.name == "weighted_levenshtein" and w.ragged
    assert w.substitution.dtype == np.float64 and np.array_equal(w.indel, [3.0, 3.0]) and w.symbols == ["x", "y"]
    assert np.array_equal(WeightedLevenshtein("xy", [[0, 2], [2, 0]]).indel, [1.0, 1.0])
    u = WeightedLevenshtein.unit("acgt")
    assert np.array_equal(u.substitution, 1.0 - np.eye(4)) and np.array_equal(u.indel, np.ones(4))
    z = WeightedLevenshtein("ab", [[-0.0, 1], [1, 0.0]])          # (a negative zero is a zero)
    assert not np.signbit(z.substitution).any()
    assert WeightedLevenshtein(wc.SYMBOLS, 1.0 - np.eye(128)).indel.shape == (128,)


def test_pack_coded_strings_round_trip():
    from annchor_amd.distances import encode_strings, pack_coded_strings

    X = ["bca", "", "c", "abcabc", ""]
    codes, offs, lens = pack_coded_strings(X, "abc")
    assert codes.dtype == np.uint8 and offs.dtype == np.int64 and lens.dtype == np.int32
    assert list(lens) == [3, 0, 1, 6, 0] and list(offs) == [0, 3, 3, 4, 10] and list(codes) == [1, 2, 0, 2, 0, 1, 2, 0, 1, 2]
    # the alphabet's order gives the codes, whatever the code points are; symbols beyond latin-1; a sequence of symbols
    codes, _, _ = pack_coded_strings(["zaλ", "λλ"], ["λ", "z", "a"])
    assert list(codes) == [1, 2, 0, 0, 0]
    codes, offs, lens = pack_coded_strings(["", ""], "ab")
    assert codes.size == 0 and list(lens) == [0, 0] and list(offs) == [0, 0]
    codes, _, lens = pack_coded_strings(np.array(["ab", "b"]), "ab")          # (an array of str)
    assert list(codes) == [0, 1, 1]
    long = wc.one_of_each_length([2048], 128, seed=1)
    codes, _, lens = pack_coded_strings(long + ["a"], wc.SYMBOLS)
    assert list(lens) == [2048, 1] and np.array_equal(codes[:2048], [wc.SYMBOLS.index(ch) for ch in long[0]])
    # encode_strings stays what it was: codes by the symbols present
    c, o, L, A = encode_strings(["bca", "c"])
    assert A == 3 and list(c) == [1, 2, 0, 2]


@pytest.mark.parametrize("X, alphabet, match", [
    (["abc", "abd", "abc"], "abc", r"weighted_levenshtein: string 1 holds the symbol 'd', which is not in the alphabet"),
    (["", "ab", "aλ"], "ab", r"weighted_levenshtein: string 2 holds the symbol 'λ', which is not in the alphabet"),
    (["abc", "A"], "abc", r"weighted_levenshtein: string 1 holds the symbol 'A'"),
    (["a", "b" * 2049], "ab", r"weighted_levenshtein: string 1 has 2049 symbols; at most 2048"),
    (["a", b"ab"], "ab", r"weighted_levenshtein: string 1 is a bytes, not a str"),
    (["a", 3], "ab", r"weighted_levenshtein: string 1 is a int, not a str"),
    (["a", None], "ab", r"weighted_levenshtein: string 1 is a NoneType, not a str"),
    ([np.array([0, 1]), "ab"], "ab", r"weighted_levenshtein: string 0 is a ndarray, not a str"),
    ([], "ab", r"weighted_levenshtein: no strings"),
])
def test_pack_coded_strings_refuses(X, alphabet, match):
    from annchor_amd.distances import pack_coded_strings

    with pytest.raises(ValueError, match=match):
        pack_coded_strings(X, alphabet)


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    costs = wc.dyadic(4)
    f = get_function_from_input("weighted_levenshtein", wc.kwargs_of(costs))
    assert isinstance(f, distances.WeightedLevenshtein) and isinstance(f, distances.DeviceMetric)
    assert f.name == "weighted_levenshtein" and f.ragged
    assert np.array_equal(f.substitution, costs.S) and np.array_equal(f.indel, costs.g) and "".join(f.symbols) == costs.alphabet
    h = get_function_from_input("weighted_levenshtein", {"alphabet": "ab", "substitution": [[0, 2], [2, 0]]})
    assert np.array_equal(h.indel, [1.0, 1.0])
    assert not hasattr(distances, "weighted_levenshtein")          # no default costs, no module-level instance
    for kw in (None, {}, {"alphabet": "ab"}, {"substitution": [[0, 1], [1, 0]]}):
        with pytest.raises(AssertionError, match="weighted_levenshtein metric requires alphabet and substitution kwargs"):
            get_function_from_input("weighted_levenshtein", kw)
    with pytest.raises(ValueError, match="weighted_levenshtein: substitution has shape"):
        get_function_from_input("weighted_levenshtein", {"alphabet": "abc", "substitution": [[0, 1], [1, 0]]})
    with pytest.raises(AssertionError, match="The string must be one of"):
        get_function_from_input("weighted-levenshtein", None)


def test_fit_data_is_usable():
    """The fit data set of the GPU tests: finite distances, a zero diagonal, distinct off-diagonal distances within every row (the
    index comparisons rest on no tie rule), and the host pipeline runs on it without the sampler's refusal."""
    from oracle import annchor_oracle as O

    X, costs = wc.fit_strings(), wc.fit_costs()
    nx = len(X)
    assert nx == 240 and min(map(len, X)) >= 20 and max(map(len, X)) <= 60 and len(set("".join(X))) == 12
    assert wc.metric_of(costs).metric_violation() is None
    iu = np.triu_indices(nx)
    T = np.zeros((nx, nx))
    T[iu] = wc.wed_pairs_host(X, np.stack(iu, axis=1), costs)
    T.T[iu] = T[iu]
    assert np.all(np.isfinite(T)) and np.all(np.diag(T) == 0.0)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)
    rng = np.random.default_rng(7)
    a, b, c = rng.integers(0, nx, size=(3, 5000))
    assert np.all(T[a, c] <= (T[a, b] + T[b, c]) * (1 + 1e-12))
    ora = O.OracleAnnchor(nx, lambda IJ: T[IJ[:, 0], IJ[:, 1]], **wc.FIT_CFG).fit()
    assert ora.neighbor_graph[0].shape == (nx, wc.FIT_CFG["n_neighbors"])
