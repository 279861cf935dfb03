"""The max-min anchor pick on the exact-OT routes (csrc/emd.hip), called directly: pick_anchors_maxmin(5, first) on data sets of
130 members -- three lane-strided trips of the fused pick's scan over the previous row, the last one partial.

k_emd_ns and k_emd_wide derive the anchor of round r from row r - 1 themselves (PairSource::pick_*): rounds 1 and 2 restart the
running minimum (pick_reset = 1), rounds 3 and 4 continue it.  k_emd_points does not fuse: its rounds are followed by the
picker's own arg-max launch.  In every data set members 7 and 90 are identical and carry their mass far from all others, and
the first anchor lies in the bulk, so round 0's maximum is attained twice and the first index has to win.

What is compared: the anchors with the host loop of MaxMinAnchorPicker.get_anchors (pickers.py, the D[1:] quirk included) run on
the downloaded rows; the rows with pick_anchors_selected on a fresh engine, bit for bit, and with the oracle to the bar the
route has in the file that tests it today (1e-12 up to 64 bins, test_gpu_parity.py; 1e-11 for lists, wide and point solves,
test_gpu_parity.py, test_wasserstein_wide_gpu.py, test_emd_points_gpu.py).  Coordinates stay in [0, 10), the scale of those
files: the pricing tolerance of the simplex kernels is 2^-43 x the largest ground cost.

The pick on every other route (picker.hip's own kernels, the fused Levenshtein launches, the streamed and row-sharded forms):
test_anchor_pick_gpu.py, on the tied data of anchor_pick_cases.py."""
import numpy as np
import pytest

import emd_points_cases as ec
import pool_cases as pc
from oracle import metrics as om

pytestmark = pytest.mark.gpu

NX, NA, FIRST = 130, 5, 3
TWIN, TWIN2 = 7, 90


def _masses(rng, k, integral):
    return rng.integers(1, 40, k).astype(np.float64) if integral else rng.random(k) + 0.01


def _plane_cost(rng, nbulk, nfar):
    """Bins on the plane: nbulk of them in [0, 4)^2, then nfar in [9, 10)^2."""
    pts = np.concatenate([rng.random((nbulk, 2)) * 4, 9 + rng.random((nfar, 2))])
    return np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))


def _histograms(rng, nb, bulk, far, kmin, kmax, kfar, integral):
    """NX rows of kmin .. kmax entries on the bins `bulk`; the twins hold kfar entries on the bins `far`."""
    X = np.zeros((NX, nb))
    for i in range(NX):
        k = int(rng.integers(kmin, kmax + 1))
        X[i, rng.choice(bulk, k, replace=False)] = _masses(rng, k, integral)
    X[TWIN] = 0
    X[TWIN, rng.choice(far, kfar, replace=False)] = _masses(rng, kfar, integral)
    X[TWIN2] = X[TWIN]
    return X


def _histogram_route(M, X, wide, atol, oracle=None):
    from annchor_amd.distances import Wasserstein

    H = oracle if oracle is not None else om.Histograms(X, M)
    return dict(bind=lambda eng: Wasserstein(M, wide=wide).bind(eng, X), pairs=H.pairs, atol=atol, argmax_launches=0)


def ns_dense(integral):
    """k_emd_ns, cost matrix in LDS: 16 bins on a line, cost |a - b|."""
    rng = np.random.default_rng(100 + integral)
    M = np.abs(np.subtract.outer(np.arange(16.0), np.arange(16.0)))
    X = _histograms(rng, 16, np.arange(10), np.arange(13, 16), 1, 8, 2, integral)
    return _histogram_route(M, X, False, 1e-12)


def ns_sparse(integral):
    """k_emd_ns on (bin, mass) lists: 200 bins, at most 32 entries per row."""
    rng = np.random.default_rng(110 + integral)
    M = _plane_cost(rng, 180, 20)
    X = _histograms(rng, 200, np.arange(180), np.arange(180, 200), 1, 32, 10, integral)
    assert (X != 0).sum(1).max() == 32
    return _histogram_route(M, X, False, 1e-11)


def wide_dense(integral):
    """k_emd_wide on dense rows: 100 bins, rows of more than 32 entries."""
    rng = np.random.default_rng(120 + integral)
    M = _plane_cost(rng, 80, 20)
    X = _histograms(rng, 100, np.arange(80), np.arange(80, 100), 20, 60, 15, integral)
    assert (X != 0).sum(1).max() > 32
    return _histogram_route(M, X, True, 1e-11)


def wide_lists(integral):
    """k_emd_wide on (bin, mass) lists: 400 bins, at most 128 entries per row.  The supports come from a set B of 256 bins, so
    the truth is the oracle (at most 256 bins) on X[:, B] with M[B][:, B], as in test_wasserstein_wide_gpu.py."""
    rng = np.random.default_rng(130 + integral)
    M = _plane_cost(rng, 380, 20)
    bulk, far = np.arange(236), np.arange(380, 400)
    X = _histograms(rng, 400, bulk, far, 20, 128, 15, integral)
    X[0] = 0
    X[0, rng.choice(bulk, 128, replace=False)] = _masses(rng, 128, integral)
    assert (X != 0).sum(1).max() == 128
    B = np.concatenate([bulk, far])
    return _histogram_route(M, X, True, 1e-11, oracle=om.Histograms(X[:, B], M[np.ix_(B, B)]))


def points():
    """k_emd_points: clouds of 5 .. 40 points of dim 2, float64."""
    rng = np.random.default_rng(140)
    X = [rng.random((int(L), 2)) * 4 for L in rng.integers(5, 41, NX)]
    X[TWIN] = 9 + rng.random((12, 2))
    X[TWIN2] = X[TWIN].copy()
    assert all(x.dtype == np.float64 for x in X)
    return dict(clouds=X, pairs=lambda IJ: ec.emd_pairs_host(X, IJ), atol=ec.ATOL, argmax_launches=NA - 1)


ROUTES = {"ns_dense": ns_dense, "ns_sparse": ns_sparse, "wide_dense": wide_dense, "wide_lists": wide_lists}
CASES = [(name, integral) for name in ROUTES for integral in (True, False)] + [("points", None)]


def _engine(route):
    from annchor_amd import _native

    if "clouds" in route:
        return pc.bound("emd", route["clouds"])
    eng = _native.Engine(0)
    route["bind"](eng)
    return eng


def host_anchors(D, first):
    """The loop of MaxMinAnchorPicker.get_anchors over given rows D[nx, na]: the anchor of round 1 is the arg-max of row 0; from
    then on of the running minimum that restarts WITHOUT row 0; np.argmax takes the first index."""
    chosen, spread, ix = [], None, int(first)
    for rnd in range(D.shape[1]):
        chosen.append(ix)
        row = D[:, rnd]
        if rnd == 0:
            ix = int(np.argmax(row))
        else:
            spread = row.copy() if spread is None else np.minimum(spread, row)
            ix = int(np.argmax(spread))
    return np.array(chosen, dtype=np.int64)


@pytest.mark.parametrize("name,integral", CASES, ids=["%s-%s" % (n, {True: "int", False: "float", None: "f64"}[i]) for n, i in CASES])
def test_maxmin_pick(name, integral):
    from annchor_amd import _native

    route = points() if name == "points" else ROUTES[name](integral)
    eng = _engine(route)
    eng.prof_enable(True)
    eng.prof_reset()
    eng.pick_anchors_maxmin(NA, FIRST)
    eng.synchronize()
    prof = eng.prof_get()
    eng.prof_enable(False)
    A = np.asarray(eng.download(_native.F_A)).copy()
    D = np.asarray(eng.download(_native.F_D)).reshape(NX, NA).copy()
    eng.close()
    assert np.all(np.isfinite(D)), "a failed solve (NaN)"
    # the pick: the host loop on the same rows; round 0's maximum is a real tie and its first index wins
    assert np.array_equal(A, host_anchors(D, FIRST)), (A, host_anchors(D, FIRST))
    top = np.flatnonzero(D[:, 0] == D[:, 0].max())
    assert len(top) >= 2 and top[0] == TWIN and TWIN2 in top, top
    assert A[0] == FIRST and A[1] == TWIN
    # the rows: one value per pair whether the launch derived its anchor or was handed it
    e2 = _engine(route)
    e2.pick_anchors_selected([int(a) for a in A])
    D2 = np.asarray(e2.download(_native.F_D)).reshape(NX, NA).copy()
    e2.close()
    assert np.array_equal(D, D2)
    # ... and the oracle's
    for col, a in enumerate(A):
        want = route["pairs"](np.stack([np.full(NX, a), np.arange(NX)], axis=1))
        worst = float(np.abs(D[:, col] - want).max())
        print("%s round %d, anchor %d: largest difference from the oracle %.3g" % (name, col, a, worst))
        np.testing.assert_allclose(D[:, col], want, rtol=0, atol=route["atol"])
    # who picked: the histogram kernels themselves, the picker's arg-max launch after each round but the last on point clouds
    launches = prof.get("maxmin_argmax", {"launches": 0})["launches"]
    assert launches == route["argmax_launches"], prof
