"""The pair-list form above 256 anchors (up to the cap, 1024): nearest-anchor sets wider than four mask words
(csrc/locality.hip, csrc/enemies.hip: the "wide" kernels) and the tiled feature kernel for them (csrc/features.hip:
k_features_wide), every stage against the oracle.

Input sizes, checked on the CPU with the oracle's MaxMin anchors (pairs of the oracle's list, shortest row; for the strings
also the oracle fit's time and peak memory on one CPU core):
  float64, 3000 x 8 uniform (seed 1), 1024 anchors, locality 5:  108 856 pairs, shortest row 23.
  strings (1600), 300 anchors, locality 40:  300 506 pairs, shortest row 199,  4 s,  2.9 GB.
  strings (1600), 600 anchors, locality 40:  274 067 pairs, shortest row 190, 14 s,  5.3 GB.
  strings (1600), 300 anchors, locality 5:   835 056 pairs, shortest row 488, 20 s,  8.0 GB.
  strings (1600), 600 anchors, locality 5: 1 267 260 pairs, shortest row 996, 41 s, 24.0 GB.
The string cases are the ones the feature's specification names (1600 strings; 300 and 600 anchors; locality 5 and 40 with
loc_thresh = max(1, locality // 4)).  They exceed its guide of 2 x 10^5 oracle pairs: at loc_thresh 1 every string shares
one of its five nearest anchors with hundreds of others (integer distances, ties to the smaller anchor index), and no
parameter left free (seed, n_neighbors, loc_min) shrinks the list.  They are kept as specified; the figures above are what
they cost."""
import numpy as np
import pytest

from oracle import annchor_oracle as O
from oracle import metrics as om
from test_gpu_parity import _staged_compare

pytestmark = pytest.mark.gpu

CAP = 1024


@pytest.fixture(scope="module")
def strings():
    return om.load_strings()[0]


# niters: 1 where the first iteration's budget refines every pair (600 anchors, locality 40: 177 250 pairs not computed after
# the features, a budget of ~250 000 per iteration) -- the oracle then stops sampling, and _staged_compare steps through niters
@pytest.mark.parametrize("n_anchors,locality,niters", [(300, 5, 2), (300, 40, 2), (600, 5, 2), (600, 40, 1)])
def test_fit_wide_anchors_strings_stagewise(strings, n_anchors, locality, niters):
    """Levenshtein on the 1600 strings: A, D, IJs, I, features, ncm, samples, thresholds, bounds and the graph bit for bit.
    p_work 0.7 lies above the budget floor (about 0.68 at 300 anchors and 900 samples); at 600 anchors the budget raises it
    to 1."""
    from annchor_amd import Annchor

    Xs = list(strings)
    cfg = dict(n_anchors=n_anchors, n_neighbors=10, n_samples=900, p_work=0.7, random_seed=7, niters=niters, locality=locality,
               loc_thresh=max(1, locality // 4))
    ann = Annchor(np.array(Xs), "levenshtein", **cfg)
    P = om.PackedStrings(Xs)
    _staged_compare(ann, lambda tr: O.OracleAnnchor(len(Xs), P.pairs, trace=tr, **cfg))
    want = O.nearest_anchor_sets(ann.D, locality)
    assert all(set(a) == set(b) for a, b in zip(ann.sid, want))
    ann._engine.close()


@pytest.fixture(scope="module")
def fitted_1024():
    """float64 points, 1024 anchors: every stage against the oracle (the tolerances of _staged_compare)."""
    from annchor_amd import Annchor

    X = np.random.default_rng(1).uniform(size=(3000, 8))
    # (sampler: the oracle's default, the reference's draw; at 4.5 x 10^6 point pairs Annchor would pick its device sampler)
    cfg = dict(n_anchors=CAP, n_neighbors=10, n_samples=900, p_work=0.5, random_seed=3, niters=1, locality=5, loc_thresh=1,
               loc_min=20, sampler="legacy")
    ann = Annchor(X, "euclidean", **cfg)
    traces = []

    def oracle(tr):
        traces.append(tr)
        return O.OracleAnnchor(len(X), lambda IJ: om.euclidean_pairs(X, IJ), trace=tr, **cfg)

    ora = _staged_compare(ann, oracle, float_metric=True)
    assert ora.p_work == 1   # (the budget rule at this size)
    # the features as computed (one iteration: no bound updates since), to the metric tolerance _staged_compare applies to D:
    # 3000 points end inside a 64-column word and 1024 anchors are 32 full anchor chunks of k_features_wide
    np.testing.assert_allclose(ann.features, traces[0]["features"]["features"], rtol=1e-14, atol=0)
    return X, ann


def test_fit_1024_anchors_float64_stagewise(fitted_1024):
    X, ann = fitted_1024
    assert ann.n_anchors == CAP and ann.D.shape == (len(X), CAP)


def test_sets_1024_anchors(fitted_1024):
    _, ann = fitted_1024
    sid = ann.sid
    want = O.nearest_anchor_sets(ann.D, 5)
    assert len(sid) == len(want)
    assert all(set(a) == set(b) for a, b in zip(sid, want))


def _fitted_state(ann, X):
    """An oracle object holding the device's fitted state (the pattern of tests/test_enemies.py::oracle_from_state)."""
    o = O.OracleAnnchor.__new__(O.OracleAnnchor)
    o.nx, o.n_anchors, o.locality, o.loc_thresh = len(X), ann.n_anchors, ann.locality, ann.loc_thresh
    o.metric_pairs = lambda IJ: om.euclidean_pairs(X, np.asarray(IJ, dtype=np.int64))
    o.A, o.D = np.asarray(ann.A, dtype=np.int64), np.array(ann.D)
    o.sid = O.nearest_anchor_sets(o.D, ann.locality)
    o.IJs, o.I_ptr, o.I_idx = np.array(ann.IJs), np.array(ann.I.ptr), np.array(ann.I.idx)
    o.features, o.RA, o.ncm = np.array(ann.features), np.array(ann.RefineApprox), np.array(ann.not_computed_mask, dtype=bool)
    r = ann.regression
    o.bins, o.W, o.c = np.array(r.sample_bins), np.array(r.coef_), np.array(r.intercept_)
    o.errs = [np.asarray(ann.error_predictor.errs[lab], dtype=np.float64) for lab in ann.error_predictor.labels]
    return o


def test_query_1024_anchors(fitted_1024):
    """Annchor.query on the 1024-anchor fit against the oracle's query on the same fitted state: the comparison of
    test_query_matches_oracle_strings (evaluations, indices, distances; distances to _staged_compare's metric tolerance)."""
    X, ann = fitted_1024
    Q = np.random.default_rng(2).uniform(size=(60, 8))
    gi, gd = ann.query(Q, nn=5, p_work=0.4)   # (above the floor Annchor.query applies: 0.344 here)
    o = _fitted_state(ann, X)
    XQ = np.concatenate([X, Q])
    oi, od, info = O.query(o, lambda IJ: om.euclidean_pairs(XQ, np.stack([IJ[:, 0], IJ[:, 1] + len(X)], 1)), len(Q), nn=5,
                           p_work=0.4)
    assert ann.query_evals == info["evals"]
    assert np.array_equal(gi, oi)
    np.testing.assert_allclose(gd, od, rtol=1e-14, atol=0)


def test_nearest_enemies_1024_anchors(fitted_1024):
    """get_nearest_enemies on the 1024-anchor fit against the oracle's nearest_enemies on the same fitted state: the new
    pairs, the not-computed mask and the graph."""
    X, ann = fitted_1024
    y = (X[:, 0] + X[:, 1] > 1.0).astype(np.int64)
    o = _fitted_state(ann, X)
    n0 = len(o.IJs)
    oi, od = O.nearest_enemies(o, y, nn=2, loc_min=100)
    ann.get_nearest_enemies(y, nn=2, loc_min=100)
    gi, gd = ann.nearest_enemy_graph
    assert np.array_equal(ann.IJs[n0:], o.IJs[n0:])
    assert np.array_equal(ann.not_computed_mask, o.ncm)
    assert np.array_equal(gi, oi)
    np.testing.assert_allclose(gd, od, rtol=1e-14, atol=0)


def test_anchor_cap():
    """cap + 1 anchors: ANNCHOR_ELIMIT (-4), and the message names the cap."""
    from annchor_amd import Annchor

    X = np.random.default_rng(4).uniform(size=(CAP + 200, 3))
    ann = Annchor(X, "euclidean", n_anchors=CAP + 1, n_neighbors=5, n_samples=500, p_work=0.5)
    with pytest.raises(RuntimeError, match=r"error -4: n_anchors=%d: this build supports 1\.\.%d" % (CAP + 1, CAP)):
        ann.get_anchors()
