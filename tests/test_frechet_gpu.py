"""The discrete Frechet distance on the device (csrc/seqdp.hip): its cases of the small- and boundary-length sections; the
other sections are test_seqdp_gpu.py's."""
import numpy as np
import pytest

import seqdp_cases as sc
import test_seqdp_gpu as suite

pytestmark = pytest.mark.gpu

S = suite.BY_NAME["frechet"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim, longest", [(2, 96), (1, 40), (3, 40), (4, 40)])
def test_small_lengths(dim, longest, dtype):
    X = sc.one_of_each_length(range(1, longest + 1), dim, seed=40 + dim, dtype=dtype)
    suite.small_lengths(S, X, (dim, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", sc.DIMS)
def test_boundary_lengths(dim, shape, dtype):
    suite.boundary_lengths(S, dim, shape, dtype)
