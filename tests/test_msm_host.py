"""Move-Split-Merge on the host: seqdp_cases.py's sweep with MSM's measure and its lane-by-lane restatement of the kernel's
schedule (csrc/seqdp.hip) against the plain double loop, the known answers, the textbook form, symmetry, the triangle inequality,
parameter validation, pack_msm_series and the name lookup."""
import numpy as np
import pytest

import elastic_cases as lc
import seqdp_cases as sc

KNOWN = [
    ([1, 2, 3], [2, 2, 2], 0.5, 2.0),
    ([0], [4], 1.0, 4.0),
    ([1, 1, 1, 5], [1, 5], 0.25, 0.5),
    ([3, 1, 4, 1, 5], [2, 7, 1], 1.0, 11.0),
]


def mixed_series(seed):
    """Random walks, tie data of both kinds and float32 members, lengths 1..12 and a few up to 70."""
    lengths = list(range(1, 13)) + [31, 47, 70]
    rng = np.random.default_rng(seed)
    return ([rng.standard_normal(L) for L in lengths] + lc.tie_series("ints", lengths, seed + 1)
            + lc.tie_series("grid", lengths, seed + 2) + [rng.standard_normal(L).astype(np.float32) for L in lengths[::3]])


@pytest.mark.parametrize("c", [1.0, 0.37])
def test_helper_equals_the_double_loop(c):
    """All ordered pairs (both argument orders), bit for bit; symmetric and zero on the diagonal."""
    X = mixed_series(1)
    IJ = lc.all_ordered_pairs(len(X))
    got = lc.msm_pairs_host(X, IJ, c)
    want = np.array([lc.msm_loop(X[i], X[j], c) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)


@pytest.mark.parametrize("x, y, c, want", KNOWN)
def test_known_answers(x, y, c, want):
    x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
    for a, b in ((x, y), (y, x)):
        assert lc.msm_loop(a, b, c) == want
        assert lc.msm_textbook(a, b, c) == want
        assert lc.msm_pairs_host([a, b], [[0, 1]], c)[0] == want


def test_textbook_form_equals_the_inf_boundary_form():
    """M(0, 0) = |x0 - y0| and a first row and column of running sums of C, against +inf boundaries and virtual points at 0.0."""
    X = mixed_series(2)
    rng = np.random.default_rng(3)
    for i, j in rng.integers(0, len(X), size=(400, 2)):
        assert lc.msm_textbook(X[i], X[j], 0.37) == lc.msm_loop(X[i], X[j], 0.37)


def test_ties_take_the_first_case():
    """v == a, v == b and a == b: C is c."""
    for v, a, b in ((1.0, 1.0, 3.0), (3.0, 1.0, 3.0), (2.0, 2.0, 2.0), (1.0, 1.0, 0.0), (0.0, -0.0, 5.0), (-0.0, 0.0, -5.0)):
        assert lc.msm_cost(v, a, b, 0.3) == 0.3 == lc.msm_cost(v, b, a, 0.3)
        assert sc._msm_cost_v(np.float64(v), np.float64(a), np.float64(b), np.float64(0.3)) == 0.3
    assert lc.msm_cost(4.0, 1.0, 3.0, 0.25) == 1.25 == lc.msm_cost(4.0, 3.0, 1.0, 0.25)
    assert lc.msm_cost(0.0, 1.0, 3.0, 0.25) == 1.25


def test_triangle_inequality():
    """d(a, c) <= d(a, b) + d(b, c) + 1e-12 on 30 short series (values rounded to one decimal, so that many sums tie): a sanity
    bound on rounding, not a measurement."""
    rng = np.random.default_rng(0)
    S = [rng.normal(size=rng.integers(1, 9)).round(1) for _ in range(30)]
    n = len(S)
    D = lc.msm_pairs_host(S, lc.all_ordered_pairs(n), 0.5).reshape(n, n)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0)
    excess = D[:, None, :] - (D[:, :, None] + D[None, :, :])
    assert excess.max() <= 1e-12


def test_pack_msm_series():
    from annchor_amd.distances import MSM_MAX_LENGTH, pack_msm_series

    assert MSM_MAX_LENGTH == sc.max_length("msm", 1) == 2048
    rng = np.random.default_rng(3)
    cur = [rng.standard_normal(L) for L in (1, 5, 2048, 17)]
    values, offs, lens = pack_msm_series(cur)
    assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32
    assert list(lens) == [1, 5, 2048, 17] and list(offs) == [0, 1, 6, 2054]
    assert np.array_equal(values, np.concatenate(cur))
    assert pack_msm_series([s.astype(np.float32) for s in cur])[0].dtype == np.float32
    assert pack_msm_series([cur[0].astype(np.float32), cur[1]])[0].dtype == np.float64
    X2 = rng.standard_normal((4, 9))
    v, o, L = pack_msm_series(X2)
    assert np.array_equal(v.reshape(4, 9), X2) and list(L) == [9] * 4


@pytest.mark.parametrize("bad, match", [
    ([np.ones(3), np.ones((3, 2))], "msm: series 1 has 2 dimensions; univariate series only"),
    ([np.ones((3, 1)), np.ones(3)], "msm: series 0 has 2 dimensions; univariate series only"),
    ([np.ones(3), np.zeros(0)], "msm: series 1 is empty"),
    ([np.ones(2049), np.ones(3)], "msm: series 0 has 2049 values; at most 2048"),
    ([np.ones(3), np.ones(2), np.ones(2049)], "msm: series 2 has 2049 values; at most 2048"),
    ([np.array(["a", "b"]), np.ones(3)], "msm: series 0 has dtype"),
    ([np.array([1.0, np.nan]), np.ones(3)], "msm: series 0 .*not finite"),
    ([np.ones(3), np.ones(4), np.array([1.0, np.inf])], "msm: series 2 .*not finite"),
])
def test_pack_msm_series_refuses(bad, match):
    from annchor_amd.distances import pack_msm_series

    with pytest.raises(ValueError, match=match):
        pack_msm_series(bad)


@pytest.mark.parametrize("c", [np.nan, np.inf, -np.inf, 0.0, -1.0, 0, "0.5", None, 1j, True])
def test_c_must_be_a_finite_number_above_zero(c):
    from annchor_amd.distances import MSM

    with pytest.raises(ValueError, match="msm: c must be a finite real number > 0"):
        MSM(c=c)


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("msm", None)
    assert f is distances.msm and isinstance(f, distances.MSM) and isinstance(f, distances.DeviceMetric)
    assert f.name == "msm" and f.ragged and f.c == 1.0
    assert get_function_from_input("msm", {}) is distances.msm
    h = get_function_from_input("msm", {"c": 0.5})
    assert isinstance(h, distances.MSM) and h is not distances.msm and h.c == 0.5
    assert distances.MSM(c=np.float32(2)).c == 2.0 and distances.MSM(c=3).c == 3.0
    with pytest.raises(ValueError, match="finite real number"):
        get_function_from_input("msm", {"c": np.nan})


# ---------------------------------------------------------------------------------------- the kernel's schedule, restated
@pytest.mark.parametrize("kind", ["walk", "ints"])
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_lane_by_lane_restatement_equals_the_double_loop(shape, kind):
    """The schedule of k_seqdp<T, 1, R, G, MsmOp> on 64 lanes -- both wavefront shifts, the strip, the point above a lane's first
    row (the origin on lane 0 of every group) and the previous column's point (the origin at column 0) -- against msm_loop, for
    every (R, G): lengths 1, 2, R-1, R, R+1, 2R, GR-1, GR at the narrow shapes and 1, R+1, limit-1, limit at the widest, all
    crossed, inactive slots in the last wavefront of the 4-pairs shape."""
    R, G = sc.instantiations("msm", 1)[shape]
    Ls, IJ = sc.lane_case("msm", 1, shape)
    X = lc.tie_series(kind, Ls, seed=60 + shape)
    got = lc.msm_lanes(X, IJ, 0.37, R, G)
    want = lc.msm_pairs_host(X, IJ, 0.37) if shape == 2 else np.array([lc.msm_loop(X[i], X[j], 0.37) for i, j in IJ])
    if shape == 2:   # (the double loop on the short partners; the long pairs through the helper the tests above tie to it)
        short = np.flatnonzero((IJ < 2).any(axis=1))
        assert np.array_equal(want[short], [lc.msm_loop(X[i], X[j], 0.37) for i, j in IJ[short]])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
