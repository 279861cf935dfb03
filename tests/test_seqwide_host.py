"""The host side of DTW(wide=True) and Frechet(wide=True): the packers' limits and wording, the spellings of utils, the constants."""
import numpy as np
import pytest

from annchor_amd import distances
from annchor_amd.utils import get_function_from_input

PACKERS = [("dtw", "series", distances.pack_dtw_series_wide), ("frechet", "curve", distances.pack_curves_wide)]


@pytest.mark.parametrize("metric, noun, pack", PACKERS)
def test_packers(metric, noun, pack):
    rng = np.random.default_rng(1)
    z = lambda L, dim: rng.standard_normal((L, dim))
    for match, X in [("%s: %s 0 has dim 65; dim 1 .. 64 is supported" % (metric, noun), [z(3, 65), z(3, 65)]),
                     ("%s: %s 1 has 1025 points; at most 1024 are supported at dim 13" % (metric, noun), [z(3, 13), z(1025, 13)]),
                     ("%s: %s 0 has 2049 points; at most 2048 are supported at dim 2" % (metric, noun), [z(2049, 2), z(3, 2)]),
                     ("%s: %s 1 has dim 6, %s 0 has dim 5" % (metric, noun, noun), [z(3, 5), z(3, 6)]),
                     ("%s: %s 1 is empty" % (metric, noun), [z(3, 5), np.zeros((0, 5))]),
                     ("%s: %s 1 holds a value that is not finite" % (metric, noun), [z(3, 5), np.full((2, 5), np.inf)])]:
        with pytest.raises(ValueError, match=match):
            pack(X)
    values, offs, lens, dim = pack([z(1024, 64).astype(np.float32), z(1, 64).astype(np.float32)])
    assert values.dtype == np.float32 and values.size == 1025 * 64 and dim == 64
    assert offs.tolist() == [0, 1024] and lens.tolist() == [1024, 1]
    assert pack([z(2048, 2), z(5, 2)])[3] == 2   # (up to 4 coordinates: the narrow limits)


def test_constants_and_spellings():
    assert distances.DTW_WIDE_MAX_DIM == distances.FRECHET_WIDE_MAX_DIM == 64 and distances.DTW_MAX_DIM == distances.FRECHET_MAX_DIM == 4
    assert get_function_from_input("dtw", None) is distances.dtw and get_function_from_input("frechet", None) is distances.frechet
    assert get_function_from_input("dtw", {}) is distances.dtw and get_function_from_input("frechet", {"wide": False}) is distances.frechet
    assert not distances.dtw.wide and not distances.frechet.wide and not distances.DTW(window=3).wide
    m = get_function_from_input("dtw", {"wide": True, "window": 6})
    assert isinstance(m, distances.DTW) and m.wide and m.window == 6
    m = get_function_from_input("dtw", {"wide": True})
    assert m.wide and m.window is None
    m = get_function_from_input("dtw", {"window": 2})
    assert not m.wide and m.window == 2
    m = get_function_from_input("frechet", {"wide": True})
    assert isinstance(m, distances.Frechet) and m.wide
