"""Wasserstein(M, wide=True): exact solves of up to 256 nodes (k_emd_wide, csrc/emd.hip) against the oracle's shortest-path
solver, which works on the full, unreduced LP.

Tolerance: the project's bar for more than 64 bins, atol=1e-11 with rtol=0 (test_gpu_parity.py).  Measured on the CPU before
the kernel ran: a sequential restatement of the kernel's pivoting rules (tools/sim/emd_wide_sim.py) differed from the oracle
by at most 7.1e-15 on sixty pairs of 100 .. 256 nodes (integral and float masses), so the bar needs no widening for 256-node
solves.

A solve that runs into its pivot cap or meets a broken tree (any tree walk longer than the node count) writes NaN and raises
the sticky `fail` flag -- every failure path does both; the flag is not readable from the host, the NaN is, so "no NaN" is the
check for both."""
import numpy as np
import pytest

from oracle import metrics as om

pytestmark = pytest.mark.gpu

ATOL = 1e-11
NB, NX = 256, 120
# rows built by hand (the rest are random): supports that put a pair on a slot boundary of the kernel (64 nodes per slot)
R_A, R_B = 0, 1            # bins 0..127 against 128..255: 256 nodes
R_33, R_32 = 2, 3          # 33 + 32 = 65
R_64A, R_64B, R_65 = 4, 5, 6   # 64 + 64 = 128, 64 + 65 = 129
R_96A, R_96B, R_97 = 7, 8, 9   # 96 + 96 = 192, 96 + 97 = 193
R_ONE, R_REST = 10, 11     # one bin against the 255 others: a star, and its transpose
R_ID0, R_ID1 = 12, 13      # identical rows
R_HALF, R_TWICE = 14, 15   # identical after normalisation
R_FULL0, R_FULL1 = 16, 17  # full supports that differ on 40 bins only: 40 nodes after the common mass cancels
HAND = [(R_A, R_B), (R_B, R_A), (R_33, R_32), (R_64A, R_64B), (R_64A, R_65), (R_96A, R_96B), (R_96A, R_97), (R_97, R_96A),
        (R_ONE, R_REST), (R_REST, R_ONE), (R_ID0, R_ID1), (R_TWICE, R_HALF), (R_FULL0, R_FULL1), (R_FULL1, R_FULL0),
        (R_A, R_REST), (R_A, R_A)]
HAND_NODES = {(R_A, R_B): 256, (R_33, R_32): 65, (R_64A, R_64B): 128, (R_64A, R_65): 129, (R_96A, R_96B): 192,
              (R_96A, R_97): 193, (R_ONE, R_REST): 256, (R_FULL0, R_FULL1): 40}


def _cloud(rng, nb):
    pts = rng.random((nb, 2)) * 10
    return np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))


def _masses(rng, k, integral):
    return rng.integers(1, 40, k).astype(np.float64) if integral else rng.random(k) + 0.01


def _slot_data(integral):
    rng = np.random.default_rng(40 + integral)
    M = _cloud(rng, NB)
    X = np.zeros((NX, NB))
    for i in range(NX):
        k = int(rng.integers(20, 150))
        X[i, rng.choice(NB, k, replace=False)] = _masses(rng, k, integral)

    def block(row, lo, hi):
        X[row] = 0
        X[row, lo:hi] = _masses(rng, hi - lo, integral)

    block(R_A, 0, 128); block(R_B, 128, 256)
    block(R_33, 0, 33); block(R_32, 33, 65)
    block(R_64A, 0, 64); block(R_64B, 64, 128); block(R_65, 64, 129)
    block(R_96A, 0, 96); block(R_96B, 96, 192); block(R_97, 96, 193)
    X[R_ONE] = 0; X[R_ONE, 5] = 3.0 if integral else 0.7
    block(R_REST, 0, 256); X[R_REST, 5] = 0
    X[R_ID1] = X[R_ID0]
    X[R_TWICE] = 2.0 * X[R_HALF]
    # (multiples of 1/64 in the float case: the two row sums are then equal exactly, and only the 40 changed bins are left)
    X[R_FULL0] = rng.integers(2, 40, NB) / (1.0 if integral else 64.0)
    X[R_FULL1] = X[R_FULL0]
    ch = rng.choice(NB, 40, replace=False)
    X[R_FULL1, ch[:20]] += 1.0 if integral else 1.0 / 64.0
    X[R_FULL1, ch[20:]] -= 1.0 if integral else 1.0 / 64.0
    IJ = np.concatenate([np.array(HAND), rng.integers(0, NX, (300, 2))])
    H = om.Histograms(X, M)
    return dict(X=X, M=M, IJ=IJ, H=H, want=H.pairs(IJ))


_CACHE = {}


def slot_data(integral):
    if integral not in _CACHE:
        _CACHE[integral] = _slot_data(integral)
    return _CACHE[integral]


def _nodes(X, i, j):
    d = X[i] / X[i].sum() - X[j] / X[j].sum()
    return int((d != 0).sum())


def _refused(f, X, match, exc=Exception):
    """bind() must refuse X; the engine is closed either way."""
    from annchor_amd import _native

    eng = _native.Engine(0)
    try:
        with pytest.raises(exc, match=match):
            f.bind(eng, X)
    finally:
        eng.close()


def _bound(M, X, wide=True):
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    eng = _native.Engine(0)
    Wasserstein(M, wide=wide).bind(eng, X)
    return eng


@pytest.mark.parametrize("integral", [True, False])
def test_slot_boundaries_against_the_oracle(integral):
    """256 bins on a 2-d point cloud: solves of exactly 65, 128, 129, 192, 193 and 256 nodes, a 1 x 255 star and its transpose,
    identical rows (exactly 0), full supports that cancel down to 40 nodes, 300 random pairs."""
    d = slot_data(integral)
    X = d["X"]
    for (i, j), want_nodes in HAND_NODES.items():
        assert _nodes(X, i, j) == want_nodes, (i, j)
    eng = _bound(d["M"], X)
    got = eng.metric_pairs(d["IJ"])
    eng.close()
    assert np.all(np.isfinite(got)), "a solve hit its pivot cap (NaN: the fail flag was raised)"
    print("largest difference from the oracle: %.3g" % np.abs(got - d["want"]).max())
    np.testing.assert_allclose(got, d["want"], rtol=0, atol=ATOL)
    for pair in [(R_ID0, R_ID1), (R_TWICE, R_HALF), (R_A, R_A)]:
        assert got[HAND.index(pair)] == 0.0, pair


@pytest.mark.parametrize("integral", [True, False])
def test_one_to_all_form(integral):
    """pick_anchors_selected: the one-to-all launches of the anchor rounds, from the 128-entry row and from a random one."""
    from annchor_amd import _native

    d = slot_data(integral)
    eng = _bound(d["M"], d["X"])
    anchors = (R_A, 40)
    eng.pick_anchors_selected(list(anchors))
    D = eng.download(_native.F_D).reshape(NX, 2)
    eng.close()
    assert np.all(np.isfinite(D))
    for col, a_ in enumerate(anchors):
        want = d["H"].pairs(np.stack([np.full(NX, a_), np.arange(NX)], axis=1))
        np.testing.assert_allclose(D[:, col], want, rtol=0, atol=ATOL)


@pytest.mark.parametrize("integral", [True, False])
def test_lists_beyond_256_bins(integral):
    """400 bins, supports of up to 128 entries, all drawn from one set B of 256 bins: the LP only sees the supports, so the
    truth is the oracle (at most 256 bins) on X[:, B] with M[B][:, B].  Includes a 128 + 128 disjoint pair (256 nodes)."""
    rng = np.random.default_rng(50 + integral)
    nb, nx = 400, 60
    M = _cloud(rng, nb)
    B = np.sort(rng.choice(nb, 256, replace=False))
    X = np.zeros((nx, nb))
    for i in range(nx):
        k = int(rng.integers(1, 129))
        X[i, rng.choice(B, k, replace=False)] = _masses(rng, k, integral)
    X[0] = 0; X[0, B[:128]] = _masses(rng, 128, integral)
    X[1] = 0; X[1, B[128:]] = _masses(rng, 128, integral)
    X[2] = 0; X[2, B[::2]] = _masses(rng, 128, integral)      # interleaved with X[3]: the lists' merge
    X[3] = 0; X[3, B[1::2]] = _masses(rng, 128, integral)
    X[4] = X[2]; X[4, B[0]] += 1.0                            # shares 128 bins with X[2]
    X[5] = 0; X[5, B[200]] = 1.0
    IJ = np.concatenate([np.array([[0, 1], [1, 0], [2, 3], [2, 4], [4, 2], [5, 0], [0, 5], [3, 3], [0, 2]]),
                         rng.integers(0, nx, (150, 2))])
    want = om.Histograms(X[:, B], M[np.ix_(B, B)]).pairs(IJ)
    eng = _bound(M, X)
    got = eng.metric_pairs(IJ)
    eng.close()
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    assert got[7] == 0.0


@pytest.mark.parametrize("integral", [True, False])
def test_bland_fallback(monkeypatch, integral):
    """Bland's rule from the first pivot (ANNCHOR_EMD_DANTZIG_CAP=0): the hand-built pairs and 20 random ones."""
    monkeypatch.setenv("ANNCHOR_EMD_DANTZIG_CAP", "0")
    d = slot_data(integral)
    k = len(HAND) + 20
    eng = _bound(d["M"], d["X"])
    got = eng.metric_pairs(d["IJ"][:k])
    eng.close()
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, d["want"][:k], rtol=0, atol=ATOL)


def _sparse_200(integral):
    """The data of test_wasserstein_more_than_64_bins_sparse: 200 bins, at most 32 entries per histogram."""
    rng = np.random.default_rng(5 + integral)
    nb, nx = 200, 400
    pts = rng.random((nb, 2)) * 10
    M = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    X = np.zeros((nx, nb))
    for i in range(nx):
        k = int(rng.integers(1, 33))
        centre = rng.integers(0, nb)
        near = np.argsort(M[centre])[:60]
        sup = rng.choice(near, k, replace=False)
        X[i, sup] = rng.integers(1, 40, k) if integral else rng.random(k) + 0.01
    return X, M, rng


def test_unchanged_routes():
    """Data the narrow binding takes is evaluated by the same kernels through the wide one: bit-equal values on the digits
    (64 bins) and on 200-bin, 32-entry lists; and without `wide` a 40-entry row is still refused."""
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    dg = om.load_digits()
    rng = np.random.default_rng(3)
    for X, M in [(dg["X"], dg["cost_matrix"])] + [_sparse_200(integral)[:2] for integral in (True, False)]:
        IJ = rng.integers(0, X.shape[0], (2000, 2))
        e0, e1 = _bound(M, X, wide=False), _bound(M, X, wide=True)
        a, b = e0.metric_pairs(IJ), e1.metric_pairs(IJ)
        e0.close(); e1.close()
        assert np.array_equal(a, b)
    X, M, _ = _sparse_200(True)
    Xbad = X.copy(); Xbad[0, :40] = 1.0
    _refused(Wasserstein(M), Xbad, "32 non-zero")


def test_refusals_of_the_wide_binding():
    from annchor_amd import _native
    from annchor_amd.distances import Wasserstein

    rng = np.random.default_rng(6)
    M = _cloud(rng, 400)
    X = np.zeros((4, 400)); X[:, :10] = 1.0
    X[1, :129] = 1.0
    _refused(Wasserstein(M, wide=True), X, r"error -4: .*at most 128 non-zero entries.*256 nodes.*129", _native.NativeError)
    M2 = _cloud(rng, 1025)
    X2 = np.zeros((4, 1025)); X2[:, :10] = 1.0
    _refused(Wasserstein(M2, wide=True), X2, r"error -4: .*1025.*1\.\.1024 bins", _native.NativeError)
    X3, M3, _ = _sparse_200(True)
    _refused(Wasserstein(M3 ** 2, wide=True), X3, r"error -4: .*metric ground cost.*64 bins", _native.NativeError)


def grid_data():
    """250 histograms on a 12 x 12 grid (144 bins, Euclidean ground cost), blobs of 40 .. 90 lit pixels."""
    rng = np.random.default_rng(8)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    M = np.sqrt(((g[:, None] - g[None]) ** 2).sum(-1))
    nx = 250
    X = np.zeros((nx, 144))
    for i in range(nx):
        k = int(rng.integers(40, 91))
        centre = rng.random(2) * 11
        w = np.exp(-((g - centre) ** 2).sum(-1) / (2 * rng.uniform(2.0, 4.0) ** 2)) + 1e-3
        sup = rng.choice(144, k, replace=False, p=w / w.sum())
        X[i, sup] = rng.integers(1, 30, k)
    return X, M


def test_plumbing_fit_brute_force_query_and_loose_calls():
    from annchor_amd import Annchor, BruteForce, compare_neighbor_graphs
    from annchor_amd.distances import Wasserstein

    X, M = grid_data()
    nx = X.shape[0]
    kw = {"cost_matrix": M, "wide": True}
    ann = Annchor(X, "wasserstein", func_kwargs=kw, n_anchors=8, n_neighbors=6, n_samples=300, p_work=0.6, random_seed=1).fit()
    bf = BruteForce(X, "wasserstein", func_kwargs=kw).fit(6)
    assert np.all(np.isfinite(bf.neighbor_graph[1]))
    assert compare_neighbor_graphs(bf.neighbor_graph, ann.neighbor_graph, 6) <= 0.03 * nx * 6
    H = om.Histograms(X, M)
    rows = np.arange(0, nx, 10)
    IJ = np.stack([np.repeat(rows, 5), bf.neighbor_graph[0][rows, 1:].ravel()], axis=1)
    np.testing.assert_allclose(bf.neighbor_graph[1][rows, 1:].ravel(), H.pairs(IJ), rtol=0, atol=ATOL)
    qi, qd = ann.query(X[:10], nn=5)
    assert np.array_equal(np.asarray(qi)[:, 0], np.arange(10))
    assert np.all(np.asarray(qd)[:, 0] == 0)
    # loose objects
    f = Wasserstein(M, wide=True)
    want = H.pairs(np.array([[0, 1], [0, 2], [0, 3]]))
    assert abs(f(X[0], X[1]) - want[0]) <= ATOL
    np.testing.assert_allclose(f.many([X[0], X[0]], [X[1], X[2]]), want[:2], rtol=0, atol=ATOL)
    np.testing.assert_allclose(f.one_to_many(X[0], [X[1], X[2], X[3]]), want, rtol=0, atol=ATOL)
    # nearest enemies: two classes
    y = (np.arange(nx) % 2).astype(np.int64)
    ann.get_nearest_enemies(y, nn=3)
    ei, ed = ann.nearest_enemy_graph
    assert np.all(y[np.asarray(ei)] != y[:, None])
    assert np.all(np.isfinite(ed))
