"""The discrete Frechet distance on the host: seqdp_cases.py's sweep with Frechet's measure against the plain double loop, the known
answers, the triangle inequality on the fit data, pack_curves, the name lookup, and the fit data set's usability (the CPU
restatement of the pipeline accepts it, and no row of its distance matrix holds a tie)."""
import numpy as np
import pytest

import dtw_cases as dc
import frechet_cases as fc
from oracle import annchor_oracle as O

_FIT = {}


def fit_matrix():
    """Every pair of the fit data set, [nx, nx], computed once (i <= j, mirrored: the transposed matrix of the recurrence has the
    same cells; test_helper_equals_the_double_loop checks both orders against the loop)."""
    if "T" not in _FIT:
        X = fc.fit_curves()
        nx = len(X)
        iu = np.triu_indices(nx)
        T = np.zeros((nx, nx))
        T[iu] = fc.frechet_pairs_host(X, np.stack(iu, axis=1))
        T.T[iu] = T[iu]
        T.setflags(write=False)
        _FIT["T"] = T
    return _FIT["T"]


@pytest.mark.parametrize("dim", fc.DIMS)
def test_helper_equals_the_double_loop(dim):
    """All length pairs in 1..12 and a few up to 70, both argument orders (all ordered pairs), float64 and float32 members, bit
    for bit."""
    rng = np.random.default_rng(dim)
    lengths = list(range(1, 13)) + [31, 47, 70]
    cur = [rng.standard_normal((L, dim)) for L in lengths] + [rng.standard_normal((L, dim)).astype(np.float32) for L in lengths]
    IJ = fc.all_ordered_pairs(len(cur))
    got = fc.frechet_pairs_host(cur, IJ)
    want = np.array([fc.frechet_loop(cur[i], cur[j]) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(cur), -1), got.reshape(len(cur), -1).T)


@pytest.mark.parametrize("x, y, want", [
    ([(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (2, 1)], 1.0),
    ([0, 1, 2], [0, 2], 1.0),
    ([(3, 4)], [(0, 0)], 5.0),
    ([(0, 0)], [(3, 4), (6, 8)], 10.0),
    ([0, 0, 0], [1, 1, 1], 1.0),
])
def test_known_answers(x, y, want):
    x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
    for a, b in ((x, y), (y, x)):
        assert fc.frechet_loop(a, b) == want
        assert fc.frechet_pairs_host([a, b], [[0, 1]])[0] == want


def test_known_answers_against_dtw_and_self():
    """[0,0,0] against [1,1,1]: the Frechet distance is the largest step, 1; DTW sums the three, sqrt(3).  A curve against
    itself is at 0."""
    assert dc.dtw_loop([0, 0, 0], [1, 1, 1]) == np.sqrt(3.0)
    assert fc.frechet_loop([0, 0, 0], [1, 1, 1]) == 1.0
    rng = np.random.default_rng(2)
    for dim in fc.DIMS:
        cur = [rng.standard_normal((L, dim)) for L in (1, 2, 9, 37)]
        assert all(fc.frechet_loop(c, c) == 0.0 for c in cur)
        assert np.all(fc.frechet_pairs_host(cur, np.stack([np.arange(4), np.arange(4)], 1)) == 0.0)


def test_triangle_inequality_on_the_fit_data():
    """d(a, c) <= (d(a, b) + d(b, c)) (1 + 1e-12) for 5000 random triples: the slack is far above the few ulps that the rounding
    of c(i, j) and of the square root can cost.  This checks the mathematics (and the data), not the kernel."""
    T = fit_matrix()
    rng = np.random.default_rng(7)
    a, b, c = rng.integers(0, len(T), size=(3, 5000))
    assert np.all(T[a, c] <= (T[a, b] + T[b, c]) * (1 + 1e-12))


def test_pack_curves_round_trip():
    from annchor_amd.distances import pack_curves

    rng = np.random.default_rng(3)
    cur = [rng.standard_normal((L, 2)) for L in (1, 5, 2048, 17)]
    values, offs, lens, dim = pack_curves(cur)
    assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32 and dim == 2
    assert list(lens) == [1, 5, 2048, 17] and list(offs) == [0, 1, 6, 2054]
    for s, o, L in zip(cur, offs, lens):
        assert np.array_equal(values[o * 2:(o + L) * 2].reshape(L, 2), s)
    v32, _, _, _ = pack_curves([s.astype(np.float32) for s in cur])
    assert v32.dtype == np.float32
    vmix, _, _, _ = pack_curves([cur[0].astype(np.float32), cur[1]])
    assert vmix.dtype == np.float64 and np.array_equal(vmix[:2], cur[0].astype(np.float32).ravel())
    vint, _, _, _ = pack_curves([np.arange(6).reshape(3, 2), cur[1]])
    assert vint.dtype == np.float64
    # dim 3 and 4 up to 1024 points
    for d in (3, 4):
        v, o, L, dd = pack_curves([rng.standard_normal((1024, d)), rng.standard_normal((3, d))])
        assert dd == d and list(L) == [1024, 3] and list(o) == [0, 1024] and v.shape == (1027 * d,)
    # 1-D members: curves of dim 1; a [len, 1] member is the same thing
    v, o, L, d = pack_curves([np.array([1.0, 2.0, 3.0]), np.array([[4.0], [5.0]])])
    assert d == 1 and list(v) == [1, 2, 3, 4, 5] and list(o) == [0, 3] and list(L) == [3, 2]
    # a 3-D array: nx curves of equal length
    X3 = rng.standard_normal((4, 9, 3)).astype(np.float32)
    v, o, L, d = pack_curves(X3)
    assert v.dtype == np.float32 and d == 3 and np.array_equal(v.reshape(4, 9, 3), X3) and list(o) == [0, 9, 18, 27]
    assert list(L) == [9] * 4
    # a 2-D array: nx univariate rows, as for DTW
    X2 = rng.standard_normal((4, 9))
    v, o, L, d = pack_curves(X2)
    assert v.dtype == np.float64 and d == 1 and np.array_equal(v.reshape(4, 9), X2) and list(o) == [0, 9, 18, 27]
    assert list(L) == [9] * 4


@pytest.mark.parametrize("bad, match", [
    ([np.ones((3, 2)), np.ones((3, 3))], "curve 1 has dim 3, curve 0 has dim 2"),
    ([np.ones(3), np.ones((3, 2))], "curve 1 has dim 2, curve 0 has dim 1"),
    ([np.ones((3, 5)), np.ones((3, 5))], "curve 0 has dim 5"),
    ([np.ones((3, 2)), np.zeros((0, 2))], "curve 1 is empty"),
    ([np.ones((3, 2)), np.ones((2049, 2))], "curve 1 has 2049 points"),
    ([np.ones(2049), np.ones(3)], "curve 0 has 2049 points"),
    ([np.ones((1025, 3)), np.ones((3, 3))], "curve 0 has 1025 points; at most 1024 .* dim 3"),
    ([np.ones((3, 4)), np.ones((1025, 4))], "curve 1 has 1025 points; at most 1024 .* dim 4"),
    ([np.array([["a", "b"]]), np.ones((3, 2))], "curve 0 has dtype"),
    ([np.ones((3, 2)), np.ones((3, 2), dtype=complex)], "curve 1 has dtype"),
    ([np.array([[1.0, np.nan]]), np.ones((3, 2))], "curve 0 .*not finite"),
    ([np.ones((3, 2)), np.ones((4, 2)), np.array([[1.0, 2.0], [np.inf, 0.0]])], "curve 2 .*not finite"),
    ([np.ones((3, 2, 2)), np.ones((3, 2))], "curve 0 has 3 dimensions"),
])
def test_pack_curves_refuses(bad, match):
    from annchor_amd.distances import pack_curves

    with pytest.raises(ValueError, match=match):
        pack_curves(bad)


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("frechet", None)
    assert f is distances.frechet and isinstance(f, distances.Frechet) and isinstance(f, distances.DeviceMetric)
    assert f.name == "frechet" and f.ragged


def test_fit_data_is_usable():
    """The GPU fit tests' data set and configuration pass the CPU restatement of the pipeline: enough candidates for every
    point (no "Not enough candidates" error), finite distances; and within every row of the all-pairs matrix the off-diagonal
    distances are distinct, so the index comparison on the GPU rests on no tie rule."""
    X = fc.fit_curves()
    assert fc.FIT_CFG == dc.FIT_CFG
    assert len(X) == 240 and all(x.shape[1] == 2 for x in X) and min(map(len, X)) >= 20 and max(map(len, X)) <= 60
    T = fit_matrix()
    nx = len(X)
    assert np.all(np.isfinite(T)) and np.all(np.diag(T) == 0.0)
    off = T[~np.eye(nx, dtype=bool)].reshape(nx, nx - 1)
    assert all(len(np.unique(row)) == nx - 1 for row in off)
    flat = T.ravel()

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(flat[IJ[:, 0] * nx + IJ[:, 1]])

    ora = O.OracleAnnchor(nx, pairs, **fc.FIT_CFG).fit()
    assert ora.neighbor_graph[0].shape == (240, 10)
    assert np.all(np.isfinite(ora.neighbor_graph[1]))
