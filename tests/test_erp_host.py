"""Edit distance with real penalty on the host: seqdp_cases.py's sweep with ERP's measure against the plain double loop, the known
answers, the lower bound by the gap sums, the triangle inequality on the fit data, pack_erp_series, the name lookup, and the
lane-by-lane restatement of the kernel's schedule (csrc/seqdp.hip) against the double loop."""
import numpy as np
import pytest

import erp_cases as ec
import seqdp_cases as sc

_FIT = {}


def fit_matrix():
    """Every pair of the fit data set, [nx, nx], computed once (i <= j, mirrored: the transposed matrix of the recurrence has the
    same cells; test_helper_equals_the_double_loop checks both orders against the loop)."""
    if "T" not in _FIT:
        X = ec.fit_curves()
        nx = len(X)
        iu = np.triu_indices(nx)
        T = np.zeros((nx, nx))
        T[iu] = ec.erp_pairs_host(X, np.stack(iu, axis=1))
        T.T[iu] = T[iu]
        T.setflags(write=False)
        _FIT["T"] = T
    return _FIT["T"]


@pytest.mark.parametrize("gap", [0.0, 0.37])
@pytest.mark.parametrize("dim", ec.DIMS)
def test_helper_equals_the_double_loop(dim, gap):
    """All length pairs in 1..12 and a few up to 70, both argument orders (all ordered pairs), float64 and float32 members, bit
    for bit."""
    rng = np.random.default_rng(dim)
    lengths = list(range(1, 13)) + [31, 47, 70]
    cur = [rng.standard_normal((L, dim)) for L in lengths] + [rng.standard_normal((L, dim)).astype(np.float32) for L in lengths]
    IJ = ec.all_ordered_pairs(len(cur))
    got = ec.erp_pairs_host(cur, IJ, gap)
    want = np.array([ec.erp_loop(cur[i], cur[j], gap) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(cur), -1), got.reshape(len(cur), -1).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


@pytest.mark.parametrize("x, y, gap, want", [
    ([1, 2, 3], [1, 2, 3], 0.0, 0.0),
    ([1, 2, 3], [1, 3], 0.0, 2.0),
    ([3], [1, 1], 0.0, 3.0),
    ([3], [1, 1], 1.0, 2.0),
    ([[3, 4]], [[0, 0], [0, 0]], 0.0, 5.0),
])
def test_known_answers(x, y, gap, want):
    x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
    for a, b in ((x, y), (y, x)):
        assert ec.erp_loop(a, b, gap) == want
        assert ec.erp_pairs_host([a, b], [[0, 1]], gap)[0] == want


@pytest.mark.parametrize("gap", [0.0, 0.37])
def test_lower_bound_by_the_gap_sums(gap):
    """At dim 1, erp(x, y) >= | sum |x_i - g| - sum |y_j - g| | (the triangle inequality through the empty series).  Slack for
    the float sums: a cell has at most 60 + 60 additions behind it and the two sums of the bound at most 60 + 60 more, each
    rounding by at most 2^-53 relative to a value that is at most S, the two sums together: 240 x 2^-53 S < 3e-14 S."""
    rng = np.random.default_rng(11)
    X = [np.cumsum(rng.standard_normal(int(L))) for L in rng.integers(1, 61, size=80)]
    IJ = rng.integers(0, len(X), size=(1500, 2))
    d = ec.erp_pairs_host(X, IJ, gap)
    s = np.array([np.abs(x - gap).sum() for x in X])
    lb = np.abs(s[IJ[:, 0]] - s[IJ[:, 1]])
    assert np.all(d >= lb - 3e-14 * (s[IJ[:, 0]] + s[IJ[:, 1]]))
    assert np.any(lb > 1.0)


def test_triangle_inequality_on_the_fit_data():
    """d(a, c) <= (d(a, b) + d(b, c)) (1 + 1e-12) for 5000 random triples: the slack is far above the few ulps that rounding
    can cost.  This checks the mathematics (and the data), not the kernel."""
    T = fit_matrix()
    rng = np.random.default_rng(7)
    a, b, c = rng.integers(0, len(T), size=(3, 5000))
    assert np.all(T[a, c] <= (T[a, b] + T[b, c]) * (1 + 1e-12))


def test_fit_data_is_usable():
    """Finite distances, a zero diagonal, and within every row of the all-pairs matrix the off-diagonal distances are distinct,
    so the index comparisons on the GPU rest on no tie rule."""
    X = ec.fit_curves()
    T = fit_matrix()
    nx = len(X)
    assert len(X) == 240 and all(x.shape[1] == 2 for x in X) and min(map(len, X)) >= 20 and max(map(len, X)) <= 60
    assert np.all(np.isfinite(T)) and np.all(np.diag(T) == 0.0)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)


def test_pack_erp_series_round_trip():
    from annchor_amd.distances import erp_max_length, pack_erp_series

    assert [erp_max_length(d) for d in (1, 2, 3, 4)] == [2048, 1024, 1024, 1024]
    rng = np.random.default_rng(3)
    cur = [rng.standard_normal((L, 2)) for L in (1, 5, 1024, 17)]
    values, offs, lens, dim = pack_erp_series(cur)
    assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32 and dim == 2
    assert list(lens) == [1, 5, 1024, 17] and list(offs) == [0, 1, 6, 1030]
    for s, o, L in zip(cur, offs, lens):
        assert np.array_equal(values[o * 2:(o + L) * 2].reshape(L, 2), s)
    v32, _, _, _ = pack_erp_series([s.astype(np.float32) for s in cur])
    assert v32.dtype == np.float32
    vmix, _, _, _ = pack_erp_series([cur[0].astype(np.float32), cur[1]])
    assert vmix.dtype == np.float64 and np.array_equal(vmix[:2], cur[0].astype(np.float32).ravel())
    vint, _, _, _ = pack_erp_series([np.arange(6).reshape(3, 2), cur[1]])
    assert vint.dtype == np.float64
    # 1-D members: series of dim 1, up to 2048 values; a [len, 1] member is the same thing
    v, o, L, d = pack_erp_series([np.array([1.0, 2.0, 3.0]), np.array([[4.0], [5.0]])])
    assert d == 1 and list(v) == [1, 2, 3, 4, 5] and list(o) == [0, 3] and list(L) == [3, 2]
    v, o, L, d = pack_erp_series([rng.standard_normal(2048), rng.standard_normal(3)])
    assert d == 1 and list(L) == [2048, 3]
    # a 3-D array: nx series of equal length; a 2-D array: nx univariate rows
    X3 = rng.standard_normal((4, 9, 3)).astype(np.float32)
    v, o, L, d = pack_erp_series(X3)
    assert v.dtype == np.float32 and d == 3 and np.array_equal(v.reshape(4, 9, 3), X3) and list(o) == [0, 9, 18, 27]
    X2 = rng.standard_normal((4, 9))
    v, o, L, d = pack_erp_series(X2)
    assert v.dtype == np.float64 and d == 1 and np.array_equal(v.reshape(4, 9), X2) and list(L) == [9] * 4


@pytest.mark.parametrize("bad, match", [
    ([np.ones((3, 2)), np.ones((3, 3))], "erp: series 1 has dim 3, series 0 has dim 2"),
    ([np.ones(3), np.ones((3, 2))], "erp: series 1 has dim 2, series 0 has dim 1"),
    ([np.ones((3, 5)), np.ones((3, 5))], "erp: series 0 has dim 5"),
    ([np.ones((3, 2)), np.zeros((0, 2))], "erp: series 1 is empty"),
    ([np.ones(2049), np.ones(3)], "erp: series 0 has 2049 points; at most 2048 .* dim 1"),
    ([np.ones((3, 2)), np.ones((1025, 2))], "erp: series 1 has 1025 points; at most 1024 .* dim 2"),
    ([np.ones((1025, 3)), np.ones((3, 3))], "erp: series 0 has 1025 points; at most 1024 .* dim 3"),
    ([np.ones((3, 4)), np.ones((1025, 4))], "erp: series 1 has 1025 points; at most 1024 .* dim 4"),
    ([np.array([["a", "b"]]), np.ones((3, 2))], "erp: series 0 has dtype"),
    ([np.ones((3, 2)), np.ones((3, 2), dtype=complex)], "erp: series 1 has dtype"),
    ([np.array([[1.0, np.nan]]), np.ones((3, 2))], "erp: series 0 .*not finite"),
    ([np.ones((3, 2)), np.ones((4, 2)), np.array([[1.0, 2.0], [np.inf, 0.0]])], "erp: series 2 .*not finite"),
    ([np.ones((3, 2, 2)), np.ones((3, 2))], "erp: series 0 has 3 dimensions"),
])
def test_pack_erp_series_refuses(bad, match):
    from annchor_amd.distances import pack_erp_series

    with pytest.raises(ValueError, match=match):
        pack_erp_series(bad)


@pytest.mark.parametrize("gap", [np.nan, np.inf, -np.inf, "0.5", None, 1j, True])
def test_gap_must_be_a_finite_real_number(gap):
    from annchor_amd.distances import ERP

    with pytest.raises(ValueError, match="erp: gap must be a finite real number"):
        ERP(gap=gap)


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("erp", None)
    assert f is distances.erp and isinstance(f, distances.ERP) and isinstance(f, distances.DeviceMetric)
    assert f.name == "erp" and f.ragged and f.gap == 0.0
    assert get_function_from_input("erp", {}) is distances.erp
    h = get_function_from_input("erp", {"gap": 0.5})
    assert isinstance(h, distances.ERP) and h is not distances.erp and h.gap == 0.5
    assert distances.ERP(gap=np.float32(2)).gap == 2.0 and distances.ERP(gap=3).gap == 3.0
    with pytest.raises(ValueError, match="finite real number"):
        get_function_from_input("erp", {"gap": np.nan})


# ---------------------------------------------------------------------------------------- the kernel's schedule, restated
_LOOP = {}


def loop_ref(X, key, i, j, gap):
    """erp_loop on one pair of a lane case's data set, computed once per (data set, pair, gap)."""
    k = (key, i, j, gap)
    if k not in _LOOP:
        _LOOP[k] = ec.erp_loop(X[i], X[j], gap)
    return _LOOP[k]


@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", ec.DIMS)
def test_lane_by_lane_restatement_equals_the_double_loop(dim, shape):
    """The schedule of k_seqdp<T, DIM, R, G, ErpOp> on 64 lanes -- both wavefront shifts, the strip, E(-1, .) arriving at lane 0
    and E(., -1) at column -1 -- against erp_loop, for every (R, G) at every dim: lengths 1, 2, R-1, R, R+1, 2R, GR-1, GR at the
    narrow shapes and 1, R+1, limit-1, limit at the widest, all crossed, a non-zero gap, inactive slots in the last wavefront
    of the 4-pairs shape."""
    R, G = sc.instantiations("erp", dim)[shape]
    Ls, IJ = sc.lane_case("erp", dim, shape)
    gap = 0.37
    X = ec.one_of_each_length(Ls, dim, seed=60 + 10 * dim + shape)
    got = ec.erp_lanes(X, IJ, gap, R, G)
    want = np.array([loop_ref(X, (dim, shape), i, j, gap) for i, j in IJ])
    assert np.all(np.isfinite(want)) and np.all(want[IJ[:, 0] != IJ[:, 1]] > 0)
    assert np.array_equal(got, want)


def test_lane_by_lane_restatement_with_gap_zero():
    """gap = 0 (the default) at the 4-pairs shape of dim 1 and dim 2."""
    for dim in (1, 2):
        Ls, IJ = sc.lane_case("erp", dim, 0)
        X = ec.one_of_each_length(Ls, dim, seed=90 + dim)
        want = np.array([ec.erp_loop(X[i], X[j], 0.0) for i, j in IJ])
        assert np.array_equal(ec.erp_lanes(X, IJ, 0.0, 8, 16), want)
