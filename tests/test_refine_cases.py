"""tests/refine_cases.py without a GPU: the vectorised reference of update_bounds equals O.update_bounds bit for bit, and every
case, with the lookahead list the oracle's selection gives, still has the property it was built for."""
import numpy as np
import pytest

import refine_cases as R
from oracle import annchor_oracle as O
from row_paths_cases import complete_index

_made = {}


def _index(nx):
    if nx not in _made:
        _made[nx] = R.Index(*(complete_index(nx) if nx != R.HIGH else R.high_index_host()))
    return _made[nx]


def _case(name):
    if name not in _made:
        ix = _index(R.SIZES[name])
        case = R.build_case(ix, None, None, name)
        _made[name] = (ix, case, R.host_next(ix, case.RA, case.ncm, case.sel))
    return _made[name]


@pytest.mark.parametrize("name", R.CASES)
def test_case_keeps_its_property(name):
    ix, case, nxt = _case(name)
    R.check_case(case, ix, nxt)


@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_reference_equals_the_oracle(name):
    ix, case, nxt = _case(name)
    got = R.update_bounds_ref(ix.IJs, case.RA, case.ncm, ix.ptr, ix.idx, nxt, case.feats[:, 0], case.feats[:, 1])
    want = O.update_bounds(ix.IJs, case.RA, case.ncm.astype(bool), ix.ptr, ix.idx, nxt, case.feats[:, 0], case.feats[:, 1])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] != case.feats[:, 0]).any() and (got[1] != case.feats[:, 1]).any()


def test_reference_equals_the_oracle_on_long_lists():
    """A mid-size case (lists of up to 1061 entries, a subset of the not-computed pairs listed), on every fourth listed pair."""
    ix, case, nxt = _case("past_stage_64")
    nxt = nxt[::4]
    got = R.update_bounds_ref(ix.IJs, case.RA, case.ncm, ix.ptr, ix.idx, nxt, case.feats[:, 0], case.feats[:, 1])
    want = O.update_bounds(ix.IJs, case.RA, case.ncm.astype(bool), ix.ptr, ix.idx, nxt, case.feats[:, 0], case.feats[:, 1])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_high_keys_index_is_what_the_oracle_builds_on_a_sample():
    """high_index_host() groups the points by their set of nearest anchors; on a sample of points the rows equal what the
    oracle's count rule keeps (at least loc_thresh = locality common nearest anchors)."""
    ix = _index(R.HIGH)
    X, _ = R.high_points()
    cfg = R.HIGH_CFG
    _, D = O.maxmin_anchors(lambda a: np.sqrt(((X - X[a]) ** 2).sum(axis=1)), R.HIGH, cfg["n_anchors"], cfg["random_seed"])
    sid = O.nearest_anchor_sets(D, cfg["locality"])
    Am = np.zeros(D.shape, dtype=np.int32)
    np.put_along_axis(Am, sid, 1, axis=1)
    for y in (0, 1, 4711, R.SPLIT - 1, R.SPLIT, R.HIGH - 1):
        keep = np.flatnonzero(Am @ Am[y] >= cfg["loc_thresh"])
        pr = ix.IJs[ix.idx[ix.ptr[y]:ix.ptr[y + 1]]]
        assert np.array_equal(np.where(pr[:, 0] == y, pr[:, 1], pr[:, 0]), keep[keep != y])
