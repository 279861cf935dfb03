"""DTW on the host: seqdp_cases.py's sweep with DTW's measure against the plain double loop, the known answers, pack_series, the
name lookup, and the fit data set's usability (the CPU restatement of the pipeline accepts it)."""
import numpy as np
import pytest

import dtw_cases as dc
from oracle import annchor_oracle as O

WINDOWS = [None, 0, 1, 3]


@pytest.mark.parametrize("window", WINDOWS)
def test_helper_equals_the_double_loop(window):
    """All length pairs in 1..12 (n < m, n > m, n = m), bit for bit."""
    rng = np.random.default_rng(1)
    ser = [rng.standard_normal(L) for L in range(1, 13)] + [rng.standard_normal(L).astype(np.float32) for L in range(1, 13)]
    IJ = dc.all_ordered_pairs(len(ser))
    got = dc.dtw_pairs_host(ser, IJ, window)
    want = np.array([dc.dtw_loop(ser[i], ser[j], window) for i, j in IJ])
    assert np.all(np.isfinite(want))
    assert np.array_equal(got, want)


def test_known_answers():
    rng = np.random.default_rng(2)
    ser = [rng.standard_normal(37) for _ in range(6)]
    IJ = dc.all_ordered_pairs(6)
    got = dc.dtw_pairs_host(ser, IJ, 0)
    for (i, j), g in zip(IJ, got):   # window 0 on equal lengths: the diagonal only, summed left to right
        acc = 0.0
        for a, b in zip(ser[i], ser[j]):
            t = a - b
            acc = t * t + acc
        assert g == np.sqrt(acc)
    for w in WINDOWS:
        same = dc.dtw_pairs_host(ser, np.stack([np.arange(6), np.arange(6)], 1), w)
        assert np.all(same == 0.0)


def test_pack_series_round_trip():
    from annchor_amd.distances import pack_series

    rng = np.random.default_rng(3)
    ser = [rng.standard_normal(L) for L in (1, 5, 2048, 17)]
    values, offs, lens = pack_series(ser)
    assert values.dtype == np.float64 and offs.dtype == np.int64 and lens.dtype == np.int32
    assert list(lens) == [1, 5, 2048, 17]
    for s, o, L in zip(ser, offs, lens):
        assert np.array_equal(values[o:o + L], s)
    v32, _, _ = pack_series([s.astype(np.float32) for s in ser])
    assert v32.dtype == np.float32
    vmix, _, _ = pack_series([ser[0].astype(np.float32), ser[1]])
    assert vmix.dtype == np.float64
    X = rng.standard_normal((4, 9)).astype(np.float32)
    v, o, L = pack_series(X)
    assert v.dtype == np.float32 and np.array_equal(v.reshape(4, 9), X) and list(o) == [0, 9, 18, 27] and list(L) == [9] * 4


@pytest.mark.parametrize("bad, match", [
    ([np.array([1.0, np.nan]), np.ones(3)], "not finite"),
    ([np.ones(3), np.array([1.0, np.inf])], "series 1 .*not finite"),
    ([np.ones(3), np.zeros(0)], "series 1 is empty"),
    ([np.ones(2049), np.ones(3)], "2049"),
    ([np.ones((3, 2)), np.ones(3)], "univariate"),
    ([np.array(["a", "b"]), np.ones(3)], "dtype"),
])
def test_pack_series_refuses(bad, match):
    from annchor_amd.distances import pack_series

    with pytest.raises(ValueError, match=match):
        pack_series(bad)


def test_name_lookup():
    from annchor_amd import distances
    from annchor_amd.utils import get_function_from_input

    f = get_function_from_input("dtw", {"window": 2})
    assert isinstance(f, distances.DTW) and f.window == 2 and f.name == "dtw" and f.ragged
    assert get_function_from_input("dtw", None) is distances.dtw and distances.dtw.window is None
    with pytest.raises(ValueError):
        distances.DTW(window=-1)


def test_fit_data_is_usable():
    """The GPU fit tests' data set and configuration pass the CPU restatement of the pipeline: enough candidates for every
    point (no "Not enough candidates" error), something to sample in both iterations."""
    X = dc.fit_series()
    assert len(X) == 240 and min(map(len, X)) >= 20 and max(map(len, X)) <= 60
    ora = O.OracleAnnchor(len(X), lambda IJ: dc.dtw_pairs_host(X, IJ, None), **dc.FIT_CFG).fit()
    assert ora.neighbor_graph[0].shape == (240, 10)
    assert np.all(np.isfinite(ora.neighbor_graph[1]))
