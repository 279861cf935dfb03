"""Edit distance with real penalty on the device (csrc/seqdp.hip): its cases of the small- and boundary-length sections; the
other sections are test_seqdp_gpu.py's."""
import numpy as np
import pytest

import seqdp_cases as sc
import test_seqdp_gpu as suite

pytestmark = pytest.mark.gpu

S = suite.BY_NAME["erp"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim, longest, gap", [(2, 96, 0.0), (1, 40, 0.0), (3, 40, 0.0), (4, 40, 0.0), (1, 40, 0.37), (2, 96, 0.37)])
def test_small_lengths(dim, longest, gap, dtype):
    X = sc.one_of_each_length(range(1, longest + 1), dim, seed=40 + dim, dtype=dtype)
    suite.small_lengths(S, X, (dim, gap, np.dtype(dtype).name), gap=gap)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", sc.DIMS)
def test_boundary_lengths(dim, shape, dtype):
    suite.boundary_lengths(S, dim, shape, dtype)
