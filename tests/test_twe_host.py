"""Time warp edit distance on the host: seqdp_cases.py's sweep with TWE's measure and its lane-by-lane restatement of the
kernel's schedule (csrc/seqdp.hip) against the plain double loop, the known answers, symmetry, the triangle inequality, parameter
validation, pack_twe_series and the name lookup."""
import numpy as np
import pytest

import elastic_cases as lc
import seqdp_cases as sc

KNOWN = [
    ([1, 2, 3], [2, 2, 2], 0.25, 0.5, 3.0),
    ([0], [4], 0.5, 1.0, 4.0),
    ([1, 1, 1, 5], [1, 5], 0.125, 0.5, 1.75),
    ([3, 1, 4, 1, 5], [2, 7, 1], 0.5, 1.0, 19.0),
]


@pytest.mark.parametrize("nu, lam", [(0.001, 1.0), (0.37, 0.21), (0.0, 0.5)])
@pytest.mark.parametrize("dim", lc.DIMS)
def test_helper_equals_the_double_loop(dim, nu, lam):
    """All length pairs in 1..12 and a few up to 70, both argument orders (all ordered pairs), float64 members, members with
    repeated points and float32 members, bit for bit; symmetric and zero on the diagonal."""
    rng = np.random.default_rng(dim)
    lengths = list(range(1, 13)) + [31, 47, 70]
    cur = [rng.standard_normal((L, dim)) for L in lengths]
    cur = cur + lc.with_repeats(cur, seed=dim)[4:] + [rng.standard_normal((L, dim)).astype(np.float32) for L in lengths[::3]]
    IJ = lc.all_ordered_pairs(len(cur))
    got = lc.twe_pairs_host(cur, IJ, nu, lam)
    want = np.array([lc.twe_loop(cur[i], cur[j], nu, lam) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(cur), -1), got.reshape(len(cur), -1).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


@pytest.mark.parametrize("x, y, nu, lam, want", KNOWN)
def test_known_answers(x, y, nu, lam, want):
    x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
    for a, b in ((x, y), (y, x)):
        assert lc.twe_loop(a, b, nu, lam) == want
        assert lc.twe_pairs_host([a, b], [[0, 1]], nu, lam)[0] == want
    # the same series as points of dim 2 on the first axis: dist is then a square root of a square
    x2, y2 = np.stack([x, np.zeros_like(x)], 1), np.stack([y, np.zeros_like(y)], 1)
    assert lc.twe_loop(x2, y2, nu, lam) == want


@pytest.mark.parametrize("nu, lam", [(0.05, 0.7), (0.0, 0.7)])
def test_triangle_inequality(nu, lam):
    """d(a, c) <= d(a, b) + d(b, c) + 1e-12 on 30 short series (values rounded to one decimal, so that many sums tie): a sanity
    bound on rounding, not a measurement."""
    rng = np.random.default_rng(0)
    S = [rng.normal(size=rng.integers(1, 9)).round(1) for _ in range(30)]
    n = len(S)
    D = lc.twe_pairs_host(S, lc.all_ordered_pairs(n), nu, lam).reshape(n, n)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0)
    excess = D[:, None, :] - (D[:, :, None] + D[None, :, :])
    assert excess.max() <= 1e-12


def test_pack_twe_series():
    from annchor_amd.distances import erp_max_length, pack_twe_series, twe_max_length

    assert [twe_max_length(d) for d in (1, 2, 3, 4)] == [erp_max_length(d) for d in (1, 2, 3, 4)]
    assert all(twe_max_length(d) % 64 == 0 for d in (1, 2, 3, 4))
    rng = np.random.default_rng(3)
    cur = [rng.standard_normal((L, 2)) for L in (1, 5, twe_max_length(2), 17)]
    values, offs, lens, dim = pack_twe_series(cur)
    assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32 and dim == 2
    assert list(lens) == [1, 5, twe_max_length(2), 17] and list(offs) == [0, 1, 6, 6 + twe_max_length(2)]
    for s, o, L in zip(cur, offs, lens):
        assert np.array_equal(values[o * 2:(o + L) * 2].reshape(L, 2), s)
    assert pack_twe_series([s.astype(np.float32) for s in cur])[0].dtype == np.float32
    v, o, L, d = pack_twe_series([np.array([1.0, 2.0, 3.0]), np.array([[4.0], [5.0]])])
    assert d == 1 and list(v) == [1, 2, 3, 4, 5] and list(o) == [0, 3] and list(L) == [3, 2]
    X3 = rng.standard_normal((4, 9, 3)).astype(np.float32)
    v, o, L, d = pack_twe_series(X3)
    assert v.dtype == np.float32 and d == 3 and np.array_equal(v.reshape(4, 9, 3), X3) and list(o) == [0, 9, 18, 27]


def refusals():
    from annchor_amd.distances import twe_max_length as tm

    return [
        ([np.ones((3, 2)), np.ones((3, 3))], "twe: series 1 has dim 3, series 0 has dim 2"),
        ([np.ones((3, 5)), np.ones((3, 5))], "twe: series 0 has dim 5"),
        ([np.ones((3, 2)), np.zeros((0, 2))], "twe: series 1 is empty"),
        ([np.ones(tm(1) + 1), np.ones(3)], "twe: series 0 has %d points; at most %d .* dim 1" % (tm(1) + 1, tm(1))),
        ([np.ones((3, 2)), np.ones((tm(2) + 1, 2))], "twe: series 1 has %d points; at most %d .* dim 2" % (tm(2) + 1, tm(2))),
        ([np.ones((tm(3) + 1, 3)), np.ones((3, 3))], "twe: series 0 has %d points; at most %d .* dim 3" % (tm(3) + 1, tm(3))),
        ([np.ones((3, 4)), np.ones((tm(4) + 1, 4))], "twe: series 1 has %d points; at most %d .* dim 4" % (tm(4) + 1, tm(4))),
        ([np.array([["a", "b"]]), np.ones((3, 2))], "twe: series 0 has dtype"),
        ([np.array([[1.0, np.nan]]), np.ones((3, 2))], "twe: series 0 .*not finite"),
        ([np.ones((3, 2)), np.ones((4, 2)), np.array([[1.0, 2.0], [np.inf, 0.0]])], "twe: series 2 .*not finite"),
        ([np.ones((3, 2, 2)), np.ones((3, 2))], "twe: series 0 has 3 dimensions"),
    ]


@pytest.mark.parametrize("case", range(11))
def test_pack_twe_series_refuses(case):
    from annchor_amd.distances import pack_twe_series

    bad, match = refusals()[case]
    with pytest.raises(ValueError, match=match):
        pack_twe_series(bad)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -1.0, -1e-300, "0.5", None, 1j, True])
def test_parameters_must_be_finite_and_not_negative(bad):
    from annchor_amd.distances import TWE

    with pytest.raises(ValueError, match="twe: nu must be a finite real number >= 0"):
        TWE(nu=bad)
    with pytest.raises(ValueError, match="twe: lam must be a finite real number >= 0"):
        TWE(lam=bad)
    assert TWE(nu=0, lam=0).nu == 0.0


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("twe", None)
    assert f is distances.twe and isinstance(f, distances.TWE) and isinstance(f, distances.DeviceMetric)
    assert f.name == "twe" and f.ragged and f.nu == 0.001 and f.lam == 1.0
    assert get_function_from_input("twe", {}) is distances.twe
    h = get_function_from_input("twe", {"nu": 0.5, "lam": 0.25})
    assert isinstance(h, distances.TWE) and h is not distances.twe and (h.nu, h.lam) == (0.5, 0.25)
    h = get_function_from_input("twe", {"nu": 0})
    assert (h.nu, h.lam) == (0.0, 1.0)
    h = get_function_from_input("twe", {"lam": np.float32(2)})
    assert (h.nu, h.lam) == (0.001, 2.0)
    with pytest.raises(ValueError, match="finite real number"):
        get_function_from_input("twe", {"nu": np.nan})


# ---------------------------------------------------------------------------------------- the kernel's schedule, restated
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", lc.DIMS)
def test_lane_by_lane_restatement_equals_the_double_loop(dim, shape):
    """The schedule of k_seqdp<T, DIM, R, G, TweOp> on 64 lanes -- both wavefront shifts, the strip, the point above a lane's
    first row (the origin on lane 0 of every group), the previous column's point (the origin at column 0) and the distances of the
    lane's last step handed down its rows -- against the host recurrence, for every (R, G) at every dim: lengths 1, 2, R-1, R, R+1,
    2R, GR-1, GR at the narrow shapes and 1, R+1, limit-1, limit at the widest, all crossed, repeated points, inactive slots in the
    last wavefront of the 4-pairs shape."""
    R, G = sc.instantiations("twe", dim)[shape]
    Ls, IJ = sc.lane_case("twe", dim, shape)
    nu, lam = 0.37, 0.21
    X = lc.with_repeats(lc.one_of_each_length(Ls, dim, seed=60 + 10 * dim + shape), seed=dim)
    got = lc.twe_lanes(X, IJ, nu, lam, R, G)
    if shape == 2:   # (the double loop on the short partners; the long pairs through the helper the tests above tie to it)
        want = lc.twe_pairs_host(X, IJ, nu, lam)
        short = np.flatnonzero((IJ < 2).any(axis=1))
        assert np.array_equal(want[short], [lc.twe_loop(X[i], X[j], nu, lam) for i, j in IJ[short]])
    else:
        want = np.array([lc.twe_loop(X[i], X[j], nu, lam) for i, j in IJ])
    assert np.all(np.isfinite(want)) and np.all(want[IJ[:, 0] != IJ[:, 1]] > 0)
    assert np.array_equal(got, want)


def test_lane_by_lane_restatement_with_nu_zero():
    for dim in (1, 2):
        Ls, IJ = sc.lane_case("twe", dim, 0)
        X = lc.one_of_each_length(Ls, dim, seed=90 + dim)
        want = np.array([lc.twe_loop(X[i], X[j], 0.0, 1.0) for i, j in IJ])
        assert np.array_equal(lc.twe_lanes(X, IJ, 0.0, 1.0, 8, 16), want)
