"""DTW on series of 1 .. 4 coordinates per point, on the host: seqdp_cases.py's sweep and lane model with the existing Dtw measure
on curves of dim > 1 against a dim-aware double loop; pack_series' unchanged refusal of a 2-D member beside DTW.bind taking it;
the usability of the fit data.  Every comparison of distances is np.array_equal."""
import numpy as np
import pytest

import dtw_cases as dc
import frechet_cases as fc
import pool_cases as pc
import seqdp_cases as sc
import threshold_cases as tc
from oracle import annchor_oracle as O

WINDOWS = [None, 0, 5]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("dim", sc.DIMS)
def test_sweep_equals_the_double_loop(dim, window):
    lengths = list(range(1, 13)) + [31, 47, 70]
    X = sc.one_of_each_length(lengths, dim, seed=20 + dim) + sc.one_of_each_length(lengths[::3], dim, seed=30 + dim, dtype=np.float32)
    IJ = pc.all_ordered_pairs(len(X))
    got = sc.dtw_pairs_host(X, IJ, window)
    want = np.array([tc.dtw_loop(X[i], X[j], window) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(len(X), -1), got.reshape(len(X), -1).T) and np.all(got[IJ[:, 0] == IJ[:, 1]] == 0.0)
    if dim == 1:   # the univariate loop the project already has
        assert np.array_equal(want, [dc.dtw_loop(X[i][:, 0], X[j][:, 0], window) for i, j in IJ])


@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("dim", [2, 3, 4])
def test_lane_by_lane_restatement_equals_the_double_loop(dim, shape):
    """k_seqdp<T, DIM, R, G, DtwOp> at DIM > 1 on 64 lanes, on seqdp_cases.lane_case (the lane model has no band: unbanded)."""
    R, G = sc.instantiations("dtw", dim)[shape]
    Ls, IJ = sc.lane_case("dtw", dim, shape)
    X = sc.one_of_each_length(Ls, dim, seed=80 + 10 * dim + shape)
    want = sc.dtw_pairs_host(X, IJ)
    check = np.flatnonzero((IJ < 2).any(axis=1)) if shape == 2 else np.arange(len(IJ))
    assert np.array_equal(want[check], [tc.dtw_loop(X[i], X[j]) for i, j in IJ[check]])
    got = np.sqrt(sc.lanes(X, IJ, sc.Dtw(), R, G))
    assert np.array_equal(got, want)


class _Recorder:
    def __getattr__(self, name):
        def call(*args, **kw):
            self.call = (name, args, kw)
        return call


def test_pack_series_still_refuses_what_bind_now_takes():
    from annchor_amd import distances as d

    rng = np.random.default_rng(1)
    X2 = [rng.standard_normal((5, 2)), rng.standard_normal((9, 2))]
    with pytest.raises(ValueError, match="dtw: series 0 has 2 dimensions; univariate series only"):
        d.pack_series(X2)
    eng = _Recorder()
    d.DTW(window=3).bind(eng, X2)
    name, args, kw = eng.call
    assert name == "set_series_nd" and args[3] == 2 and kw == {"window": 3} and list(args[2]) == [5, 9]
    assert np.array_equal(args[0], np.concatenate([x.ravel() for x in X2]))
    # univariate data goes where it went: a list of 1-D members, and a 2-D array of rows
    for X1 in ([rng.standard_normal(5), rng.standard_normal(9)], rng.standard_normal((4, 9))):
        d.DTW().bind(eng, X1)
        assert eng.call[0] == "set_series" and eng.call[2] == {"window": None}
    # a 3-D array: nx series of equal length
    d.DTW().bind(eng, rng.standard_normal((4, 9, 3)))
    assert eng.call[0] == "set_series_nd" and eng.call[1][3] == 3 and list(eng.call[1][2]) == [9] * 4
    # mixed members are refused by the packer, with DTW's wording
    with pytest.raises(ValueError, match="dtw: series 1 has dim 2, series 0 has dim 1"):
        d.DTW().bind(eng, [rng.standard_normal(5), rng.standard_normal((9, 2))])
    assert "out of scope" not in d.DTW.__doc__.split("Limits")[0] and "Multivariate" not in d.DTW.__doc__


def test_fit_data_is_usable():
    X = fc.fit_curves()
    assert len(X) == 240 and all(x.shape[1] == 2 for x in X)
    ora = O.OracleAnnchor(len(X), lambda IJ: sc.dtw_pairs_host(X, IJ, None), **pc.FIT_CFG).fit()
    assert ora.neighbor_graph[0].shape == (240, 10)
    assert np.all(np.isfinite(ora.neighbor_graph[1]))
