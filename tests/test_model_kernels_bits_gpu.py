"""k_ols_bins and k_err_sort give the bits of the recorded build (tests/golden/model_bits.npz, written by make_model_bits.py
on an MI355X from the commit named in the fixture): coefficients, intercepts, statuses, row counts, list offsets and flags as
int64 patterns, the sample predictions, the sorted residual lists, RefineApprox and the error labels by their SHA-256.  The cases
(model_bits_cases.py) stand round every size at which the kernels change their path: the wave, the workgroup, the compaction
trips, the LDS capacity of the work matrix, the sorter's sizes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import model_bits_cases as B  # noqa: E402

_D = {}


@pytest.fixture(scope="module", autouse=True)
def _engine():
    yield
    for d in _D.values():
        d.close()
    _D.clear()


def driver():
    if "d" not in _D:
        _D["d"] = B.Driver()
    return _D["d"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(B.GOLDEN)
    assert tuple(g["cases"]) == B.CASES and len(str(g["commit"])) == 40
    return g


@pytest.mark.parametrize("name", B.CASES)
def test_same_bits_as_the_recorded_build(name, golden):
    r = driver().run(name)
    assert np.array_equal(r["shape"], golden[name + "/shape"])
    for k in B.COMPARED:
        assert np.array_equal(r[k], golden["%s/%s" % (name, k)]), (name, k)


def test_the_cases_reach_the_sizes_they_are_named_for(golden):
    """(from the fixture alone: the recorded lists have the lengths the cases were built for)"""
    for n in B.ROW_COUNTS:
        assert n in golden["rows_%d/rows" % n]
    for m in B.SAMPLE_COUNTS:
        assert golden["m_%d/shape" % m][0] == m
    assert list(golden["short_partitions/rows"]) == [5, 0, 1, 2, 8] and list(golden["short_partitions/flags"]) == [0, 2, 1]
    assert list(golden["rows_%d/flags" % (B.M.ERR_CAP + 1)]) == [0, 0, 2] and not golden["rows_%d/flags" % B.M.ERR_CAP].any()
    assert golden["inner_edge/err_ptr"][-1] == 120 + 3
    assert golden["nb64/shape"][1] == 64 and golden["nb1/shape"][1] == 1 and list(golden["c2_shape/shape"][:2]) == [5000, 7]
    assert list(golden["ties_one_value/rows"]) == [700, 60] and list(golden["zeros/rows"]) == [64, 40]


@pytest.mark.parametrize("name", ("rows_%d" % (B.OLS_LDS_ROWS + 1), "c2_shape"))
def test_two_runs_give_the_same_bits(name):
    a, b = driver().run(name), driver().run(name)
    for k in B.COMPARED:
        assert np.array_equal(a[k], b[k]), (name, k)
