"""The host side of the point-cloud earth mover's distance: the reference of emd_points_cases.py against closed forms and an LP
solver, the packing of clouds and the name lookup.  No GPU."""
import numpy as np
import pytest

import emd_points_cases as ec


# ------------------------------------------------------------------------------------------------- the host reference
@pytest.mark.parametrize("n", [1, 2, 7, 64, 128])
def test_reference_dim1_equal_sizes(n):
    """At equal sizes the optimum pairs the sorted points: mean |sort(x) - sort(y)|."""
    rng = np.random.default_rng(n)
    x, y = rng.random(n) * 10, rng.random(n) * 10
    want = float(np.mean(np.abs(np.sort(x) - np.sort(y))))
    assert abs(ec.emd_pair_host(x, y) - want) <= 1e-13
    assert abs(ec.emd_1d_closed_form(x, y) - want) <= 1e-13


@pytest.mark.parametrize("n, m", [(1, 2), (1, 128), (3, 5), (20, 30), (64, 65), (127, 128), (128, 96)])
def test_reference_dim1_unequal_sizes(n, m):
    """At unequal sizes: the integral of |F - G| between the two empirical distribution functions."""
    rng = np.random.default_rng(100 * n + m)
    x, y = rng.random(n) * 10, rng.random((m, 1)) * 10
    assert abs(ec.emd_pair_host(x, y) - ec.emd_1d_closed_form(x, y)) <= 1e-13
    assert abs(ec.emd_pair_host(y, x) - ec.emd_1d_closed_form(x, y)) <= 1e-13


def test_reference_against_linprog():
    """Ten pairs across dim 1 .. 4 against scipy's HiGHS, an integer-lattice pair with tied costs among them."""
    pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(3)
    cases = []
    for dim, (n, m) in zip((1, 2, 3, 4, 1, 2, 3, 4), [(5, 9), (20, 30), (33, 32), (64, 17), (40, 40), (128, 128), (1, 50), (12, 12)]):
        cases.append((rng.random((n, dim)) * 10, rng.random((m, dim)) * 10))
    cases.append(tuple(ec.lattice_clouds((60, 45), 2, seed=4)))
    cases.append(tuple(ec.lattice_clouds((30, 30), 3, seed=5)))
    assert len(cases) == 10
    worst = 0.0
    for x, y in cases:
        worst = max(worst, abs(ec.emd_pair_host(x, y) - ec.emd_linprog(x, y)))
    print("host reference against HiGHS: largest difference %.3g" % worst)
    assert worst <= 1e-12


def test_reference_properties():
    """Zero on a permuted copy, symmetric to rounding, the batch helper equals the single calls."""
    rng = np.random.default_rng(6)
    X = ec.random_clouds((20, 20, 31, 1), 3, seed=7)
    X[1] = X[0][rng.permutation(20)]
    assert ec.emd_pair_host(X[0], X[1]) == 0.0
    IJ = ec.all_ordered_pairs(4)
    got = ec.emd_pairs_host(X, IJ)
    assert np.array_equal(got, [ec.emd_pair_host(X[i], X[j]) for i, j in IJ])
    T = got.reshape(4, 4)
    assert np.allclose(T, T.T, rtol=0, atol=1e-13)
    # a cloud of one point: the mean distance to it
    assert abs(T[3, 2] - ec.ground_cost(X[3], X[2]).mean()) <= 1e-13


# ------------------------------------------------------------------------------------------------------- pack_clouds
def test_pack_clouds_round_trip():
    from annchor_amd.distances import EMD_MAX_DIM, EMD_MAX_POINTS, pack_clouds

    assert (EMD_MAX_DIM, EMD_MAX_POINTS) == (4, 128)
    X = ec.random_clouds((1, 128, 17, 40), 3, seed=8)
    values, offs, lens, dim = pack_clouds(X)
    assert dim == 3 and values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32
    assert lens.tolist() == [1, 128, 17, 40] and offs.tolist() == [0, 1, 129, 146]
    for s, x in enumerate(X):
        assert np.array_equal(values[offs[s] * dim:(offs[s] + lens[s]) * dim].reshape(-1, dim), x)
    # float32 stays float32 only when every cloud is; a 3-D array and univariate rows are taken
    v32 = pack_clouds([x.astype(np.float32) for x in X])[0]
    assert v32.dtype == np.float32 and np.array_equal(v32, values.astype(np.float32))
    assert pack_clouds([X[0].astype(np.float32), X[1]])[0].dtype == np.float64
    cube = np.arange(2 * 5 * 2, dtype=np.float64).reshape(2, 5, 2)
    values, offs, lens, dim = pack_clouds(cube)
    assert dim == 2 and lens.tolist() == [5, 5] and offs.tolist() == [0, 5] and np.array_equal(values, cube.ravel())
    values, offs, lens, dim = pack_clouds([np.arange(4), np.arange(6)])
    assert dim == 1 and lens.tolist() == [4, 6] and values.dtype == np.float64


def test_pack_clouds_refusals():
    from annchor_amd.distances import HAUSDORFF_MAX_POINTS, pack_clouds, pack_point_sets

    rng = np.random.default_rng(9)
    ok = rng.random((10, 2))
    with pytest.raises(ValueError, match=r"emd: cloud 1 has 129 points; at most 128"):
        pack_clouds([ok, rng.random((129, 2))])
    with pytest.raises(ValueError, match=r"emd: cloud 0 has dim 5; dim 1 \.\. 4"):
        pack_clouds([rng.random((10, 5)), rng.random((10, 5))])
    with pytest.raises(ValueError, match=r"emd: cloud 2 has dim 3, cloud 0 has dim 2"):
        pack_clouds([ok, ok, rng.random((10, 3))])
    with pytest.raises(ValueError, match=r"emd: cloud 1 is empty"):
        pack_clouds([ok, np.zeros((0, 2))])
    for bad in (np.nan, np.inf):
        x = ok.copy()
        x[4, 1] = bad
        with pytest.raises(ValueError, match=r"emd: cloud 3 holds a value that is not finite"):
            pack_clouds([ok, ok, ok, x, ok])
    with pytest.raises(ValueError, match=r"emd: cloud 1 has dtype complex128"):
        pack_clouds([ok, ok.astype(np.complex128)])
    with pytest.raises(ValueError, match=r"emd: cloud 0 has dtype"):
        pack_clouds([np.array(["a", "b"]), ok])
    with pytest.raises(ValueError, match=r"emd: no clouds"):
        pack_clouds([])
    # 128 points are taken, and the Hausdorff limit did not move
    assert pack_clouds([rng.random((128, 2)), ok])[2].tolist() == [128, 10]
    assert HAUSDORFF_MAX_POINTS == 4096
    assert pack_point_sets([rng.random((4096, 2)), ok])[2].tolist() == [4096, 10]
    with pytest.raises(ValueError, match=r"hausdorff: set 0 has 4097 points"):
        pack_point_sets([rng.random((4097, 2)), ok])


# ------------------------------------------------------------------------------------------------------- name lookup
def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("emd", None)
    assert f is distances.emd and isinstance(f, distances.PointEMD) and f.name == "emd"
    assert f.ragged is True
    assert get_function_from_input("emd", {}) is distances.emd
    # the other names resolve as before
    assert get_function_from_input("hausdorff", None) is distances.hausdorff
    assert get_function_from_input("erp", None) is distances.erp
    with pytest.raises(AssertionError, match="must be one of"):
        get_function_from_input("emd2", None)


def test_is_metric_is_unaffected():
    """The metric's name changes no default of Annchor: is_metric stays what the caller passes, True by default."""
    import inspect

    from annchor_amd import Annchor

    assert inspect.signature(Annchor.__init__).parameters["is_metric"].default is True
    for word in ("per-point weights", "more than 128 points", "more than 4 coordinates", "other ground costs", "partial or unbalanced",
                 "entropic"):
        from annchor_amd.distances import PointEMD

        assert word in " ".join(PointEMD.__doc__.split())
