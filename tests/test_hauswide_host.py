"""The host side of Hausdorff(wide=True): the packer's limits and wording, the spellings of utils, the constants."""
import numpy as np
import pytest

from annchor_amd import distances
from annchor_amd.utils import get_function_from_input


def test_packer():
    rng = np.random.default_rng(1)
    z = lambda L, dim: rng.standard_normal((L, dim))
    pack = distances.pack_point_sets_wide
    for match, X in [("hausdorff: set 0 has dim 513; dim 1 .. 512 is supported", [z(3, 513), z(3, 513)]),
                     ("hausdorff: set 1 has 4097 points; at most 4096 are supported at dim 13", [z(3, 13), z(4097, 13)]),
                     ("hausdorff: set 1 has dim 6, set 0 has dim 5", [z(3, 5), z(3, 6)]),
                     ("hausdorff: set 1 is empty", [z(3, 5), np.zeros((0, 5))]),
                     ("hausdorff: set 1 holds a value that is not finite", [z(3, 5), np.full((2, 5), np.inf)])]:
        with pytest.raises(ValueError, match=match):
            pack(X)
    values, offs, lens, dim = pack([z(4096, 512).astype(np.float32), z(1, 512).astype(np.float32)])
    assert values.dtype == np.float32 and values.size == 4097 * 512 and dim == 512
    assert offs.tolist() == [0, 4096] and lens.tolist() == [4096, 1]
    with pytest.raises(ValueError, match="hausdorff: set 0 has dim 5; dim 1 .. 4 is supported"):
        distances.pack_point_sets([z(3, 5), z(3, 5)])


@pytest.mark.parametrize("dim", [1, 4])
def test_narrow_members_pack_the_same(dim):
    rng = np.random.default_rng(2)
    X = [rng.standard_normal((L, dim)).astype(np.float32) for L in (1, 40, 4096)]
    for a, b in zip(distances.pack_point_sets_wide(X), distances.pack_point_sets(X)):
        assert np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype


def test_constants_and_spellings():
    assert distances.HAUSDORFF_WIDE_MAX_DIM == 512 and distances.HAUSDORFF_MAX_DIM == 4 and distances.HAUSDORFF_MAX_POINTS == 4096
    for kw in (None, {}, {"wide": False}):
        assert get_function_from_input("hausdorff", kw) is distances.hausdorff
    assert not distances.hausdorff.wide and not distances.Hausdorff().wide
    m = get_function_from_input("hausdorff", {"wide": True})
    assert isinstance(m, distances.Hausdorff) and m.wide
