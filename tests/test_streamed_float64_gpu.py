"""The streamed form on float64 rows (streamed='float64' / StreamedAnnchor(float64=True); csrc/rerank64.hip): the float32 pipeline
searches the centred, narrowed copy, float64 differences re-rank, a guard certifies, an exact repair does the rest.

At p_work = 1.0 EVERY row of every case must be the float64 k-NN line by float64_cases.violations64 (gamma64 = (dimp + 4) 2^-52,
derived there), on the families of streamed_cases widened to float64 and on two that float32 cannot hold (shift_1e8, near_ties:
test_streamed_float64_host.py shows that rows narrowed on the host select another graph there), one route per tile kernel of the
float32 search.  With a binding budget the lists are float64-exact re-rankings of what the budget found.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
import float64_cases as fc   # noqa: E402
import streamed_cases as sc   # noqa: E402

N = 1777
# (route, d, n_neighbors, expected kind, expected two_stage) -- the float32 search runs with float64_search_length(n_neighbors, d) entries
ROUTES = [
    ("two-stage", 128, 13, 1, True),
    ("split", 20, 8, 1, False),
    ("k-blocked", 300, 10, 1, False),
    ("exact-f32", 64, 40, 0, False),
]
_truth = {}


def _D(name, d):
    if (name, d) not in _truth:
        X = fc.family64(name, N, d)
        _truth[(name, d)] = (X, fc.sq_dists_f64(X, X, np.arange(N)))
    return _truth[(name, d)]


def _assert_exact64(X, idx, dist, k, what, rows=None, Q=None, complete=True, D=None):
    rows = np.arange(len(X) if Q is None else len(Q)) if rows is None else rows
    assert dist.dtype == np.float64 and idx.dtype == np.int64
    bad = fc.violations64(X, rows, idx[rows], dist[rows], k, Q=Q, complete=complete, D=D)
    print("%s: %d of %d rows violate" % (what, len(bad), len(rows)))
    assert bad == [], "%s: %d of %d rows, first %s" % (what, len(bad), len(rows), bad[:4])


@pytest.mark.parametrize("name", sorted(fc.FAMILIES64))
@pytest.mark.parametrize("route,d,k,kind,two_stage", ROUTES, ids=["%s-d%d-k%d" % r[:3] for r in ROUTES])
def test_routes_by_families_are_float64_exact(route, d, k, kind, two_stage, name):
    """Flagged rows of `plain`: the host statement of the guard (test_streamed_float64_host.py, exact float32 lists of the narrowed
    copy, n = 700) certifies every row on every shape; the count on the device is printed here and asserted to be fewer than n."""
    from annchor_amd.streamed import StreamedAnnchor

    X, D = _D(name, d)
    sa = StreamedAnnchor(X, n_anchors=8, n_neighbors=k, p_work=1.0, float64=True).fit()
    got = (sa._engine.stream_last_kernel(), sa._engine.stream_last_tile_kernels()[0])
    flagged, repaired = sa.rerank64_stats
    print("%s d=%d k=%d %s: kernel %d, two-stage %s, float64 guard flagged %d of %d, repaired %s" % (route, d, k, name, got[0], got[1], flagged, N, repaired))
    assert got == (kind, two_stage), "dispatch moved: %s" % (got,)
    _assert_exact64(X, *sa.neighbor_graph, k, "%s d=%d k=%d %s" % (route, d, k, name), D=D)
    if name == "near_ties":
        assert flagged > 0 and repaired, (flagged, repaired)   # the guard and the repair were really the thing tested
    if name == "plain":
        assert flagged < N


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("name", ["plain", "shift_1e8", "near_ties"])
def test_front_end(metric, name):
    """Annchor(..., streamed='float64').  Cosine: the rows are normalised in float64 (each coordinate to (d / 2 + 3) 2^-53 relative:
    the norm's sum, its root, the division), so a computed unit row is within (d / 2 + 3) 2^-53 of the true one and a distance
    |u - v| <= 2 moves by at most twice that; d^2 / 2 then moves by at most 2 (d + 6) 2^-53, plus gamma64 relative for its own sum.
    The comparison value 1 - x.y / (|x||y|) carries (d + 4) 2^-53 absolute of its own.  Tolerance: 4 (dimp + 6) 2^-53 absolute
    + gamma64 relative; a column left out may be closer than the last listed one by no more than that."""
    from annchor_amd import Annchor

    d, k = 64, 12
    X = fc.family64(name, N, d)
    if metric == "cosine" and name == "shift_1e8":
        X = X - 1e8 + 3.0      # (after normalising, a shift of 1e8 leaves nothing of the structure in ANY arithmetic: a shift of 3 does)
    ann = Annchor(X, metric, n_anchors=8, n_neighbors=k, p_work=1.0, streamed="float64").fit()
    assert ann._streamed is not None and ann._streamed.float64
    idx, dist = ann.neighbor_graph
    assert dist.dtype == np.float64 and idx.shape == (N, k)
    if metric == "euclidean":
        _assert_exact64(X, idx, dist, k, "Annchor(streamed='float64') %s" % name)
        return
    nrm = np.linalg.norm(X, axis=1)
    C = 1.0 - (X @ X.T) / (nrm[:, None] * nrm[None, :])
    dimp = sc.padded_dim(d)
    atol, rtol = 4 * (dimp + 6) * 2.0 ** -53, fc.gamma64_of(dimp)
    rows = np.arange(N)
    assert np.array_equal(idx[:, 0], rows) and np.all(dist[:, 0] == 0.0)
    assert all(len(set(r)) == k for r in idx) and np.all(np.diff(dist, axis=1) >= 0)
    true = np.take_along_axis(C, idx, 1)
    np.testing.assert_allclose(dist[:, 1:], true[:, 1:], rtol=rtol, atol=atol)
    rest = C.copy()
    np.put_along_axis(rest, idx, np.inf, 1)
    assert np.all(rest.min(axis=1) >= true[:, 1:].max(axis=1) * (1 - rtol) - atol)


@pytest.mark.parametrize("name", ["plain", "shift_1e8", "near_ties", "far_clusters"])
@pytest.mark.parametrize("d,k", [(128, 13), (64, 40)])
def test_queries(d, k, name):
    """300 perturbed rows, nn = 5 and 40, through Annchor.query: the same criteria with Q."""
    from annchor_amd import Annchor

    X = fc.family64(name, N, d)
    ann = Annchor(X, "euclidean", n_anchors=8, n_neighbors=k, p_work=1.0, streamed="float64").fit()
    rng = np.random.default_rng(4)
    rows = np.sort(rng.choice(N, 300, replace=False))
    scale = np.abs(X - X.mean(axis=0)).mean()
    Q = X[rows] + 1e-3 * scale * rng.standard_normal((300, d))
    for nn in (5, 40):
        qi, qd = ann.query(Q, nn=nn, p_work=1.0)
        print("query %s d=%d nn=%d: guard flagged %d, repaired %s" % ((name, d, nn) + ann._streamed.query_rerank64_stats))
        _assert_exact64(X, qi, qd, nn, "query %s d=%d nn=%d" % (name, d, nn), Q=Q)


def test_float32_input_is_widened():
    """float32 rows under streamed='float64' widen exactly (every float32 is a float64): the result is the float64 graph of the
    same points, and the float64 checker passes on the widened rows."""
    from annchor_amd import Annchor

    X32 = sc.family("shift_1e5", N, 20)
    ann = Annchor(X32, "euclidean", n_anchors=8, n_neighbors=8, p_work=1.0, streamed="float64").fit()
    assert ann.neighbor_graph[1].dtype == np.float64
    _assert_exact64(X32.astype(np.float64), *ann.neighbor_graph, 8, "float32 input")


def test_refusals():
    from annchor_amd import Annchor
    from annchor_amd.streamed import SingleComm, StreamedAnnchor

    X = fc.family64("plain", 1300, 64)
    with pytest.raises(ValueError):
        Annchor(X, "euclidean", streamed=True)

    class TwoRanks(SingleComm):
        rank, world = 0, 2

    with pytest.raises(NotImplementedError):
        StreamedAnnchor(X, n_neighbors=5, comm=TwoRanks(), float64=True)
    with pytest.raises(ValueError, match="n_neighbors <= 126"):
        Annchor(X, "euclidean", n_neighbors=127, p_work=1.0, streamed="float64")
    with pytest.raises(ValueError, match="n_neighbors <= 61"):
        StreamedAnnchor(fc.family64("plain", 1300, 300), n_neighbors=62, p_work=1.0, float64=True)
    sa = StreamedAnnchor(X, n_anchors=6, n_neighbors=10, p_work=1.0, float64=True).fit()
    with pytest.raises(ValueError, match="nn <= 125"):
        sa.query(X[:10], nn=126, p_work=1.0)


@pytest.mark.parametrize("name", ["plain", "shift_1e8"])
def test_budgeted_build_is_a_float64_exact_reranking(name):
    """N = 40 000, d = 64, k = 15, p_work = 0.25: every listed pair is real and its distance float64-exact to gamma64, every row
    ascends, the evaluation count stays within the budget.  Recall against the float64 truth on 600 sampled rows is printed beside
    that of a 'cast' fit of the same data.  The float32 test of this shape (test_streamed_exact_gpu.py,
    test_budgeted_builds_stay_honest_on_hard_data) sets no recall bar, so none is set here."""
    from annchor_amd.streamed import StreamedAnnchor

    n, d, k = 40000, 64, 15
    X = fc.family64(name, n, d)
    nt = (n + 127) // 128
    sa = StreamedAnnchor(X, n_anchors=16, n_neighbors=k, p_work=0.25, float64=True).fit()
    assert sa.tile_evals <= int(np.ceil(0.25 * nt)) * nt
    assert sa.rerank64_stats == (0, False)     # nothing is flagged or repaired under a binding budget
    idx, dist = sa.neighbor_graph
    rows = np.sort(np.random.default_rng(0).choice(n, 600, replace=False))
    D = fc.sq_dists_f64(X, X, rows)
    _assert_exact64(X, idx, dist, k, "budgeted %s" % name, rows=rows, complete=False, D=D)
    ti, _ = fc.truth64(X, rows, k, D=D)
    cast = StreamedAnnchor(X.astype(np.float32), n_anchors=16, n_neighbors=k, p_work=0.25).fit()
    rec = [np.mean([len(set(a) & set(b)) / float(k) for a, b in zip(g[rows], ti)]) for g in (idx, cast.neighbor_graph[0])]
    print("budgeted %s: recall@%d against the float64 truth: float64 form %.4f, 'cast' %.4f" % (name, k, rec[0], rec[1]))
