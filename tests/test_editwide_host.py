"""ERP(wide=True) and TWE(wide=True) on the host side: the packers' limits and dtype rules, construction, the string form."""
import numpy as np
import pytest

from annchor_amd import distances
from annchor_amd.utils import get_function_from_input


@pytest.mark.parametrize("name, wide, narrow", [("erp", distances.pack_erp_series_wide, distances.pack_erp_series),
                                                ("twe", distances.pack_twe_series_wide, distances.pack_twe_series)])
def test_packer_limits_and_dtypes(name, wide, narrow):
    z = np.zeros
    for dim, limit in ((1, 2048), (2, 1024), (4, 1024), (5, 1024), (64, 1024)):
        values, offs, lens, d = wide([z((limit, dim)), z((3, dim), dtype=np.float32)])
        assert (d, values.dtype, values.size, offs.tolist(), lens.tolist()) == (dim, np.float64, (limit + 3) * dim, [0, limit], [limit, 3])
        with pytest.raises(ValueError, match="%s: series 1 has %d points; at most %d are supported at dim %d" % (name, limit + 1, limit, dim)):
            wide([z((2, dim)), z((limit + 1, dim))])
    assert wide([z((2, 9), dtype=np.float32), z((1, 9), dtype=np.float32)])[0].dtype == np.float32
    for match, X in [("%s: series 0 has dim 65; dim 1 .. 64" % name, [z((2, 65))]), ("%s: series 1 has dim 6, series 0 has dim 5" % name, [z((2, 5)), z((2, 6))]),
                     ("%s: series 1 is empty" % name, [z((2, 5)), z((0, 5))]), ("%s: series 0 holds a value that is not finite" % name, [np.full((2, 5), np.inf)])]:
        with pytest.raises(ValueError, match=match):
            wide(X)
    with pytest.raises(ValueError, match="%s: series 0 has dim 5; dim 1 .. 4" % name):
        narrow([z((2, 5))])


def test_construction_and_string_form():
    assert not distances.ERP().wide and not distances.TWE().wide and not distances.erp.wide and not distances.twe.wide
    e, t = distances.ERP(0.5, wide=True), distances.TWE(0.25, lam=2.0, wide=True)
    assert (e.gap, e.wide, t.nu, t.lam, t.wide) == (0.5, True, 0.25, 2.0, True)
    for kw, want in (({"wide": True}, (0.0, True)), ({"wide": True, "gap": 0.37}, (0.37, True)), ({"gap": 0.37}, (0.37, False))):
        f = get_function_from_input("erp", kw)
        assert isinstance(f, distances.ERP) and (f.gap, f.wide) == want
    for kw, want in (({"wide": True}, (0.001, 1.0, True)), ({"wide": True, "nu": 0.37, "lam": 0.21}, (0.37, 0.21, True)), ({"lam": 0.5}, (0.001, 0.5, False))):
        f = get_function_from_input("twe", kw)
        assert isinstance(f, distances.TWE) and (f.nu, f.lam, f.wide) == want
    assert get_function_from_input("erp", None) is distances.erp and get_function_from_input("twe", {}) is distances.twe
