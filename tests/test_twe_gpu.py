"""Time warp edit distance on the device (csrc/seqdp.hip): the test it alone has, and its cases of the small- and boundary-length
sections; the other sections are test_seqdp_gpu.py's.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import elastic_cases as lc
import pool_cases as pc
import test_seqdp_gpu as suite

pytestmark = pytest.mark.gpu

S = suite.BY_NAME["twe"]
NU, LAM = suite.NU, suite.LAM


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim, longest, nu, lam", [(1, 40, 0.001, 1.0), (2, 96, 0.001, 1.0), (3, 40, 0.001, 1.0), (4, 40, 0.001, 1.0),
                                                   (1, 40, NU, LAM), (2, 96, NU, LAM)])
def test_small_lengths(dim, longest, nu, lam, dtype):
    X = lc.one_of_each_length(range(1, longest + 1), dim, seed=40 + dim, dtype=dtype)
    suite.small_lengths(S, X, (dim, nu, np.dtype(dtype).name), nu=nu, lam=lam)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", lc.DIMS)
def test_boundary_lengths(dim, shape, dtype):
    suite.boundary_lengths(S, dim, shape, dtype)


# ---------------------------------------------------------------------------------------------- 3. coincident points
@pytest.mark.parametrize("dim", lc.DIMS)
def test_coincident_points(dim):
    """About a third of the points repeat their predecessor (dist = 0 and dx = nl there), and two members are constant: lengths
    1..70 crossed (the 4-pairs shape) and, in a second data set, a few lengths up to 300 (one pair per wavefront)."""
    for tag, lengths in (("short", range(1, 71)), ("long", [1, 2, 9, 64, 129, 200, 300])):
        X = lc.with_repeats(lc.one_of_each_length(lengths, dim, seed=70 + dim), seed=dim)
        X[3] = np.repeat(X[3][:1], len(X[3]), axis=0)
        X[5] = np.zeros_like(X[5])
        IJ = lc.all_ordered_pairs(len(X))
        want = suite.ref(("twe", "repeats", dim, tag), lambda: lc.twe_pairs_host(X, IJ, NU, LAM))
        got = pc.device_pairs("twe", X, IJ, nu=NU, lam=LAM)
        assert np.array_equal(got, want)
