"""EDR(wide=True) and LCSS(wide=True) on the host side: the packers' limits, the string form, and the test data's match share."""
import numpy as np
import pytest

import threshold_cases as tc
from annchor_amd import distances
from annchor_amd.utils import get_function_from_input
from test_threshwide_gpu import EPS, proto_series


@pytest.mark.parametrize("name, wide, narrow", [("edr", distances.pack_edr_series_wide, distances.pack_edr_series),
                                                ("lcss", distances.pack_lcss_series_wide, distances.pack_lcss_series)])
def test_packer_limits(name, wide, narrow):
    z = np.zeros
    assert distances.EDR_WIDE_MAX_DIM == distances.LCSS_WIDE_MAX_DIM == 64
    for dim, limit in ((2, 2048), (4, 1024), (5, 1024), (64, 1024)):
        values, offs, lens, d = wide([z((limit, dim)), z((3, dim), dtype=np.float32)])
        assert (d, values.dtype, values.size, lens.tolist()) == (dim, np.float64, (limit + 3) * dim, [limit, 3])
        with pytest.raises(ValueError, match="%s: series 1 has %d points; at most %d are supported at dim %d" % (name, limit + 1, limit, dim)):
            wide([z((2, dim)), z((limit + 1, dim))])
    with pytest.raises(ValueError, match="%s: series 0 has dim 65; dim 1 .. 64" % name):
        wide([z((2, 65))])
    with pytest.raises(ValueError, match="%s: series 0 has dim 5; dim 1 .. 4" % name):
        narrow([z((2, 5))])


def test_string_form_passes_wide():
    e, c = get_function_from_input("edr", {"eps": 0.5, "normalize": True, "wide": True}), get_function_from_input("lcss", {"eps": 0.5, "delta": 3, "wide": True})
    assert (type(e), e.eps, e.normalize, e.wide, type(c), c.eps, c.delta, c.wide) == (distances.EDR, 0.5, True, True, distances.LCSS, 0.5, 3, True)
    assert not get_function_from_input("edr", {"eps": 0.5}).wide and not distances.LCSS(0.5).wide


@pytest.mark.parametrize("dim", [5, 13, 64])
def test_generator_match_share(dim):
    assert 0.1 < tc.match_share(proto_series([200, 129, 64], dim, seed=70 + dim), EPS) < 0.25   # 1/5 x 7/9 = 0.156
