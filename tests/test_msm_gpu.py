"""Move-Split-Merge on the device (csrc/seqdp.hip): the test it alone has, and its cases of the small- and boundary-length
sections; the other sections are test_seqdp_gpu.py's.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import elastic_cases as lc
import pool_cases as pc
import test_seqdp_gpu as suite

pytestmark = pytest.mark.gpu

S = suite.BY_NAME["msm"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("longest, c", [(40, 1.0), (96, 1.0), (40, 0.37)])
def test_small_lengths(longest, c, dtype):
    X = lc.univariate(lc.one_of_each_length(range(1, longest + 1), 1, seed=40 + longest, dtype=dtype))
    suite.small_lengths(S, X, (longest, c, np.dtype(dtype).name), c=c)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_boundary_lengths(shape, dtype):
    suite.boundary_lengths(S, 1, shape, dtype)


# ---------------------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("kind", ["ints", "grid", "walk"])
def test_tie_data(kind):
    """Values from {-1, 0, 1, 2} and from a 3-level float32 grid, so that v == a, v == b and a == b occur in most cells, and
    non-dyadic random walks, where the min is decided in the last bits: lengths 1..70 crossed (the 4-pairs shape) and, in a second
    data set, a few lengths up to 300 (one pair per wavefront)."""
    for tag, lengths in (("short", range(1, 71)), ("long", [1, 2, 9, 64, 129, 200, 300])):
        X = lc.tie_series(kind, lengths, seed=70)
        IJ = lc.all_ordered_pairs(len(X))
        want = suite.ref(("msm", "ties", kind, tag), lambda: lc.msm_pairs_host(X, IJ, 0.3))
        got = pc.device_pairs("msm", X, IJ, c=0.3)
        assert np.array_equal(got, want)
