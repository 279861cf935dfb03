"""Host statement of the streamed float64 mode (annchor_amd.streamed: narrow_centred, rerank64_lower_bound,
rerank64_certified, float64_search_length) on the hard families: the narrowing bound holds, and the certification inequality
of the guard ("float64 rows") never certifies a row whose float32-selected list differs from the float64 truth.
No GPU: the float32 search is stood in for by the exact k-NN lists of the narrowed copy, which is what the device's search
delivers up to gamma32 -- the slack the inequality carries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import float64_cases as fc   # noqa: E402
import streamed_cases as sc   # noqa: E402

from annchor_amd import streamed as st   # noqa: E402

N = 700
SHAPES = [(20, 8, 16), (64, 13, 15), (130, 10, 18)]   # (d, n_neighbors, float32 list length)


@pytest.mark.parametrize("name", sorted(fc.FAMILIES64))
def test_narrowing_bound_holds(name):
    for d in (20, 130):
        X = fc.family64(name, N, d)
        X32, e, centre = st.narrow_centred(X)
        assert X32.dtype == np.float32 and e.dtype == np.float32 and centre.shape == (d,)
        C = X - centre[None, :]
        assert np.array_equal(X32, C.astype(np.float32))
        err = np.sqrt(((C - X32.astype(np.float64)) ** 2).sum(axis=1))
        assert np.all(err <= e.astype(np.float64)), (name, d, float((err - e).max()))
        # and it is no cruder than it has to be: within a factor 1 + 2^-19 of 2^-24 |x~| (plus the subnormal term)
        assert np.all(e <= st.U32 * (1 + 2.0 ** -19) * np.sqrt((C * C).sum(axis=1)) + 2.0 ** -140)


@pytest.mark.parametrize("name", fc.BEYOND_FLOAT32)
def test_host_narrowed_rows_select_another_graph(name):
    """The point of the two extra families: the graph selected from the rows narrowed on the host, uncentred (streamed='cast'),
    is not the float64 graph."""
    for d, k in ((128, 13), (20, 8), (300, 10), (64, 40)):
        X = fc.family64(name, 1777, d)
        rows = np.arange(0, 1777, 7)
        ti, D = fc.truth64(X, rows, k)
        ci, cd = sc.brute_f64(X.astype(np.float32), rows, k)
        assert fc.violations64(X, rows, ci, sc.true_dists(X, rows, ci), k, D=D) != [], (name, d, k)
        assert any(set(a) != set(b) for a, b in zip(ti, ci))


@pytest.mark.parametrize("name", sorted(fc.FAMILIES64))
@pytest.mark.parametrize("d,k,ks", SHAPES)
def test_certified_rows_have_the_float64_list(d, k, ks, name):
    X = fc.family64(name, N, d)
    dimp = sc.padded_dim(d)
    X32, e, _ = st.narrow_centred(X)
    rows = np.arange(N)
    li, ld = sc.brute_f64(X32, rows, ks)          # the float32 search: exact lists of the narrowed copy, self first
    d_last = ld[:, -1].astype(np.float32).astype(np.float64)
    D = fc.sq_dists_f64(X, X, rows)
    cand = np.take_along_axis(D, li[:, 1:], 1)    # float64 d^2 of the listed columns
    order = np.argsort(cand, axis=1, kind="stable")
    kept = np.take_along_axis(li[:, 1:], order, 1)[:, :k - 1]
    d_k = np.sqrt(np.take_along_axis(cand, order, 1)[:, k - 2])
    cert = st.rerank64_certified(d_k, d_last, e, dimp)
    ti, _ = fc.truth64(X, rows, k, D=D)
    # (under exact ties at the K-th place several lists are the k-NN list: a list is wrong when its worst entry is farther than the truth's)
    wrong = np.take_along_axis(cand, order, 1)[:, k - 2] > np.take_along_axis(D, ti[:, -1:], 1)[:, 0]
    assert not np.any(cert & wrong), "%s d=%d: %d certified rows are not the float64 lists" % (name, d, int((cert & wrong).sum()))
    # a certified row's boundary is strict: every unlisted column is farther than the K-th entry
    rest = D.copy()
    np.put_along_axis(rest, li, np.inf, 1)
    assert np.all(np.sqrt(rest.min(axis=1))[cert] > d_k[cert])
    assert fc.violations64(X, rows[cert], np.concatenate([rows[cert, None], kept[cert]], 1),
                           np.concatenate([np.zeros((int(cert.sum()), 1)), np.sqrt(np.take_along_axis(cand, order, 1)[cert, :k - 1])], 1), k, D=D[cert]) == []
    print("%s d=%d k=%d: %d of %d rows certified, %d of the others differ" % (name, d, k, int(cert.sum()), N, int((wrong & ~cert).sum())))
    if name == "plain":
        assert cert.sum() > N // 2          # the inequality is not vacuous
    if name == "duplicates_all":
        assert cert.sum() == 0              # nothing separates identical rows


def test_search_lengths_and_refusals():
    assert st.float64_search_length(13, 128) == 15      # stays with the two-stage kernel
    assert st.float64_search_length(8, 20) == 16
    assert st.float64_search_length(10, 300) == 18
    assert st.float64_search_length(40, 64) == 48
    assert st.float64_search_length(126, 64) == 128 and st.float64_search_length(61, 300) == 63
    assert st.float64_search_length(125, 64, query=True) == 127 and st.float64_search_length(60, 300, query=True) == 62
    for args in ((127, 64), (62, 300)):
        with pytest.raises(ValueError, match="float64 streamed form keeps 2 extra"):
            st.float64_search_length(*args)
    with pytest.raises(ValueError, match="nn <= 125"):
        st.float64_search_length(126, 64, query=True)


def test_refusals_without_a_device():
    from annchor_amd import Annchor

    X = fc.family64("plain", 300, 8)
    with pytest.raises(ValueError, match="streamed='float64'"):
        Annchor(X, "euclidean", streamed=True)          # float64 under streamed=True is still refused, and says what there is

    class TwoRanks(st.SingleComm):
        rank, world = 0, 2

    with pytest.raises(NotImplementedError, match="2 ranks"):
        st.StreamedAnnchor(X, n_neighbors=5, comm=TwoRanks(), float64=True)
    with pytest.raises(ValueError, match="n_neighbors <= 126"):
        st.StreamedAnnchor(X, n_neighbors=127, float64=True)
    with pytest.raises(ValueError, match="needs a numeric"):
        Annchor([[1.0, 2.0], [3.0]], "euclidean", streamed="float64")


def test_float32_rows_widen_without_loss():
    X32 = sc.family("shift_1e5", 200, 20)
    assert np.array_equal(X32.astype(np.float64).astype(np.float32), X32)
    assert np.array_equal(np.ascontiguousarray(X32, dtype=np.float64), X32.astype(np.float64))
