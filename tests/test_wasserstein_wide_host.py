"""Wasserstein(M, wide=...): the public switch of the wide exact-OT route, without a GPU."""
import numpy as np

from annchor_amd.distances import Wasserstein
from annchor_amd.utils import get_function_from_input


def test_wide_flag_on_the_metric_object():
    M = np.abs(np.arange(5.0)[:, None] - np.arange(5.0)[None])
    assert Wasserstein(M, wide=True).wide is True
    assert Wasserstein(M).wide is False
    f = get_function_from_input("wasserstein", {"cost_matrix": M, "wide": True})
    assert isinstance(f, Wasserstein) and f.wide is True
    assert np.array_equal(f.cost_matrix, M)
    g = get_function_from_input("wasserstein", {"cost_matrix": M})
    assert isinstance(g, Wasserstein) and g.wide is False
