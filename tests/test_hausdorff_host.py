"""The Hausdorff distance on the host: the vectorised helper of hausdorff_cases.py against the definition's loop, the known
answers, pack_point_sets, the name lookup, and the usability of the GPU tests' data sets (no ties, no zeros, the CPU
restatement of the pipeline accepts the fit data)."""
import numpy as np
import pytest

import hausdorff_cases as hc
from oracle import annchor_oracle as O


def sym_matrix(X):
    """Every pair, [nx, nx]: computed for i <= j and mirrored (test_helper_equals_the_loop checks both orders)."""
    nx = len(X)
    iu = np.triu_indices(nx)
    T = np.zeros((nx, nx))
    T[iu] = hc.hausdorff_pairs_host(X, np.stack(iu, axis=1))
    T.T[iu] = T[iu]
    return T


@pytest.mark.parametrize("dim", hc.DIMS)
def test_helper_equals_the_loop(dim):
    """Ragged pairs in both orders (all ordered pairs), n = 1 and m = 1 included, float64 and float32 members, bit for bit; the
    helper in blocks of rows as well (a block size that does not divide n)."""
    rng = np.random.default_rng(dim)
    sizes = [1, 2, 3, 7, 8, 9, 23, 40]
    sets = [rng.standard_normal((L, dim)) for L in sizes] + [rng.standard_normal((L, dim)).astype(np.float32) for L in sizes]
    IJ = hc.all_ordered_pairs(len(sets))
    want = np.array([hc.hausdorff_loop(sets[i], sets[j]) for i, j in IJ])
    assert np.all(np.isfinite(want))
    got = hc.hausdorff_pairs_host(sets, IJ)
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(sets), -1), got.reshape(len(sets), -1).T)
    assert np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    old = hc.CHUNK_CELLS
    try:
        hc.CHUNK_CELLS = 3 * 23   # 3 rows at m = 23, 1 row at m = 40
        assert np.array_equal(hc.hausdorff_pairs_host(sets, IJ), want)
    finally:
        hc.CHUNK_CELLS = old


def test_known_answers():
    both = lambda x, y: (hc.hausdorff_loop(x, y), hc.hausdorff_pairs_host([x, y], [[0, 1]])[0])
    # {0} vs {0, 3} in dim 1: h(x, y) = 0, h(y, x) = 9
    assert both([0.0], [0.0, 3.0]) == (3.0, 3.0)
    assert both([0.0, 3.0], [0.0]) == (3.0, 3.0)
    assert both([(3.0, 4.0)], [(0.0, 0.0)]) == (5.0, 5.0)
    rng = np.random.default_rng(1)
    for dim in hc.DIMS:
        x = rng.standard_normal((37, dim))
        # a set against its permutation, and against itself with duplicated points
        assert both(x, x[rng.permutation(37)]) == (0.0, 0.0)
        assert both(x, np.concatenate([x, x[[5, 5, 0, 36]]])) == (0.0, 0.0)
        # a strict subset: h(x, y) = 0, the result is sqrt(h(y, x)) > 0
        sub = x[:20]
        X, Y = hc.as_set(sub), hc.as_set(x)
        assert hc._directed_loop(X, Y) == 0.0
        hyx = hc._directed_loop(Y, X)
        assert hyx > 0.0
        assert both(sub, x) == (np.sqrt(hyx), np.sqrt(hyx)) and both(x, sub) == (np.sqrt(hyx), np.sqrt(hyx))


def test_boundary_lengths_follow_the_shapes():
    assert hc.instantiations(2) == [(8, 16), (8, 64)]
    assert hc.boundary_lengths(3) == [1, 7, 8, 9, 16, 127, 128, 129, 257, 511, 512, 513, 1025, 4095, 4096]


def test_pack_point_sets_round_trip():
    from annchor_amd.distances import HAUSDORFF_MAX_DIM, HAUSDORFF_MAX_POINTS, pack_point_sets

    assert (HAUSDORFF_MAX_DIM, HAUSDORFF_MAX_POINTS) == (4, 4096)
    rng = np.random.default_rng(3)
    sets = [rng.standard_normal((L, 3)) for L in (1, 5, 4096, 17)]
    values, offs, lens, dim = pack_point_sets(sets)
    assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32 and dim == 3
    assert list(lens) == [1, 5, 4096, 17] and list(offs) == [0, 1, 6, 4102]
    for s, o, L in zip(sets, offs, lens):
        assert np.array_equal(values[o * 3:(o + L) * 3].reshape(L, 3), s)
    v32, _, _, _ = pack_point_sets([s.astype(np.float32) for s in sets])
    assert v32.dtype == np.float32
    vmix, _, _, _ = pack_point_sets([sets[0].astype(np.float32), sets[1]])
    assert vmix.dtype == np.float64 and np.array_equal(vmix[:3], sets[0].astype(np.float32).ravel())
    vint, _, _, _ = pack_point_sets([np.arange(6).reshape(2, 3), sets[1]])
    assert vint.dtype == np.float64
    # 4096 points at every dim
    for d in (1, 2, 4):
        v, o, L, dd = pack_point_sets([rng.standard_normal((4096, d)), rng.standard_normal((3, d))])
        assert dd == d and list(L) == [4096, 3] and list(o) == [0, 4096] and v.shape == (4099 * d,)
    # 1-D members: sets of dim 1; a [len, 1] member is the same thing
    v, o, L, d = pack_point_sets([np.array([1.0, 2.0, 3.0]), np.array([[4.0], [5.0]])])
    assert d == 1 and list(v) == [1, 2, 3, 4, 5] and list(o) == [0, 3] and list(L) == [3, 2]
    # a 3-D array: nx sets of equal size
    X3 = rng.standard_normal((4, 9, 3)).astype(np.float32)
    v, o, L, d = pack_point_sets(X3)
    assert v.dtype == np.float32 and d == 3 and np.array_equal(v.reshape(4, 9, 3), X3) and list(o) == [0, 9, 18, 27]
    assert list(L) == [9] * 4
    # a 2-D array: nx univariate rows
    X2 = rng.standard_normal((4, 9))
    v, o, L, d = pack_point_sets(X2)
    assert v.dtype == np.float64 and d == 1 and np.array_equal(v.reshape(4, 9), X2) and list(o) == [0, 9, 18, 27]
    assert list(L) == [9] * 4


@pytest.mark.parametrize("bad, match", [
    ([np.ones((3, 2)), np.ones((3, 3))], "hausdorff: set 1 has dim 3, set 0 has dim 2"),
    ([np.ones(3), np.ones((3, 2))], "hausdorff: set 1 has dim 2, set 0 has dim 1"),
    ([np.ones((3, 5)), np.ones((3, 5))], "hausdorff: set 0 has dim 5"),
    ([np.ones((3, 2)), np.zeros((0, 2))], "hausdorff: set 1 is empty"),
    ([np.ones((3, 2)), np.ones((4097, 2))], "hausdorff: set 1 has 4097 points; at most 4096"),
    ([np.ones(4097), np.ones(3)], "hausdorff: set 0 has 4097 points"),
    ([np.ones((3, 4)), np.ones((4097, 4))], "hausdorff: set 1 has 4097 points; at most 4096 .* dim 4"),
    ([np.array([["a", "b"]]), np.ones((3, 2))], "hausdorff: set 0 has dtype"),
    ([np.ones((3, 2)), np.ones((3, 2), dtype=complex)], "hausdorff: set 1 has dtype"),
    ([np.array([[1.0, np.nan]]), np.ones((3, 2))], "hausdorff: set 0 .*not finite"),
    ([np.ones((3, 2)), np.ones((4, 2)), np.array([[1.0, 2.0], [np.inf, 0.0]])], "hausdorff: set 2 .*not finite"),
    ([np.ones((3, 2, 2)), np.ones((3, 2))], "hausdorff: set 0 has 3 dimensions"),
    ([], "hausdorff: no sets"),
])
def test_pack_point_sets_refuses(bad, match):
    from annchor_amd.distances import pack_point_sets

    with pytest.raises(ValueError, match=match):
        pack_point_sets(bad)


def test_pack_curves_limit_did_not_move():
    from annchor_amd.distances import pack_curves

    with pytest.raises(ValueError, match="frechet: curve 1 has 2049 points; at most 2048"):
        pack_curves([np.ones((3, 2)), np.ones((2049, 2))])
    with pytest.raises(ValueError, match="frechet: curve 0 has 1025 points; at most 1024 .* dim 3"):
        pack_curves([np.ones((1025, 3)), np.ones((3, 3))])
    assert pack_curves([np.ones((2048, 2)), np.ones((3, 2))])[2].tolist() == [2048, 3]


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("hausdorff", None)
    assert f is distances.hausdorff and isinstance(f, distances.Hausdorff) and isinstance(f, distances.DeviceMetric)
    assert f.name == "hausdorff" and f.ragged
    with pytest.raises(AssertionError, match="The string must be one of"):
        get_function_from_input("hausdorf", None)


def test_fit_data_is_usable():
    """What the GPU tests rest on.  Fit data: all 28 680 off-diagonal values of the upper triangle are distinct and none is
    zero, so the index comparisons rest on no tie rule; the CPU restatement of the pipeline accepts the data set and the
    configuration.  BruteForce data: no row of its matrix has a tie."""
    X = hc.fit_sets()
    nx = len(X)
    assert nx == 240 and all(x.shape[1] == 2 for x in X) and min(map(len, X)) >= 20 and max(map(len, X)) <= 60
    T = sym_matrix(X)
    assert np.all(np.isfinite(T)) and np.all(np.diag(T) == 0.0)
    upper = T[np.triu_indices(nx, 1)]
    assert len(upper) == 28680 and len(np.unique(upper)) == 28680 and np.all(upper > 0.0)
    flat = T.ravel()

    def pairs(IJ):
        IJ = np.asarray(IJ, dtype=np.int64).reshape(-1, 2)
        return np.asarray(flat[IJ[:, 0] * nx + IJ[:, 1]])

    ora = O.OracleAnnchor(nx, pairs, **hc.FIT_CFG).fit()
    assert ora.neighbor_graph[0].shape == (240, 10)
    assert np.all(np.isfinite(ora.neighbor_graph[1]))
    B = hc.brute_sets()
    assert len(B) == 200 and all(x.shape[1] == 3 for x in B) and len({len(x) for x in B}) > 20
    TB = sym_matrix(B)
    off = TB[~np.eye(200, dtype=bool)].reshape(200, 199)
    assert all(len(np.unique(row)) == 199 for row in off)
